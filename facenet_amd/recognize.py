"""From a photograph to the embeddings of the faces in it, on the device end to end.

``FacePipeline(detector, facenet, image_options)``: the frame is uploaded once; the same device tensor goes to the detector
(`FaceDetector.detect` -> MTCNN) and to the crop kernel (`image_processing_batch`, the pixels of `image_processing` followed by the
centre cut of `image.size`), whose uint8 output goes straight to `FaceNet.evaluate`.  The network plans one launch list (and
captures one graph) per batch size, so the face batch is zero-padded up to one of `BATCH_SIZES`: photos with 1, 2 or 3 faces
share a plan.  Inference has no coupling between the images of a batch, so the padding rows change nothing.
``align=True`` (default: the `image.align` key, off when absent) replaces the box crop with the landmark alignment of DESIGN.md
section 22 (`image_processing_aligned_batch`); ``max_residual`` then drops faces whose landmarks fit the template badly.

``Gallery(embeddings, labels, names, files, metric)`` answers "who is this?" (DESIGN.md section 19): it keeps the known faces'
embeddings on the device and ``search`` returns each query's k nearest rows from one fn_gallery_search call, whose distances
are those of the validation kernels bit for bit; ``identify`` turns the nearest row into (label, name, distance, row), open-set
with a threshold (a number, or a trained FaceToFaceNormalizedEmbeddingsClassifier's) and closed-set without.
``FacePipeline.identify`` hands the network's device output straight to the search.

``Gallery.within`` is the range query: every gallery row nearer than eps as a CSR, from fn_radius_count /
fn_radius_fill, with the same distances and the same strict fp32 < as validation and identification.  ``Gallery.cluster`` runs
DBSCAN on the self-join (fn_dbscan_*) and returns a `Clustering`; ``FacePipeline.cluster`` does so for the faces of a list of
photographs without their embeddings leaving the device.

``Gallery.spanning_tree`` and ``Gallery.hdbscan`` (`hierarchy.py`): the minimum spanning tree of the rows under
the mutual-reachability distance, built on the device (fn_mst_*), and what is read from it on the host: the cut at any threshold,
the linkage matrix and HDBSCAN, which needs no threshold.

``Gallery.mates`` is the search of the open-set evaluation: every probe's nearest mate, nearest impostor and
the rank of that mate at any depth, from fn_mate_search on the same walk and the same bits; ``statistics.IdentificationCurve``
turns them into FNIR at FPIR.

``Gallery.kmeans`` and ``Gallery.ivf`` (`ivf.py`): spherical k-means on the device and the inverted-file
index it trains; an `ivf.IVFGallery` searches only the lists a query probes, with `search`'s bits.

``Gallery.quantize`` (`quantized.py`): int8 codes of the rows; a `QuantizedGallery` takes a shortlist on the
int8 MFMA, ranks it with `search`'s bits and runs the queries it cannot certify through `search` itself.

`FacePipeline` is defined here; `Gallery`, its result types and its limits live in `gallery.py`."""
from __future__ import annotations

import numpy as np
import torch

from .detectors.face_detector import image_processing_aligned_batch, image_processing_batch
from .gallery import DBSCAN_ROUNDS, MAX_EDGES, MAX_K, MAX_LENGTH, Clustering, Gallery, MateSearch, check_edges      # noqa: F401
from .hierarchy import HierarchicalClustering, SpanningTree      # noqa: F401
from .quantized import QuantizedGallery      # noqa: F401

BATCH_SIZES = (1, 4, 16, 64, 256)


def padded_batch(n: int) -> int:
    """The smallest planned batch size that holds n faces (multiples of the largest one beyond it)."""
    for size in BATCH_SIZES:
        if n <= size:
            return size
    return -(-n // BATCH_SIZES[-1]) * BATCH_SIZES[-1]


class FacePipeline:
    def __init__(self, detector, facenet, image_options, device="cuda:0", align=None, max_residual=None):
        self.detector, self.facenet, self.image_options = detector, facenet, image_options
        self.device = torch.device(device)
        self.align = bool(getattr(image_options, "align", False)) if align is None else bool(align)
        self.max_residual = max_residual

    def _frame(self, image):
        """uint8 [H, W, 3] in the detector's channel order -> the one device copy of it."""
        if torch.is_tensor(image):
            return image.to(device=self.device, dtype=torch.uint8).contiguous()
        arr = np.ascontiguousarray(np.asarray(image, dtype=np.uint8))
        return torch.from_numpy(arr if arr.flags.writeable else arr.copy()).to(self.device)

    def crops(self, image):
        """-> (list of BoundingBox, device uint8 [F, size, size, 3]); with `align`, the faces that `aligned_crops` keeps."""
        if self.align:
            return self.aligned_crops(image)[:2]
        frame = self._frame(image)
        boxes = self.detector.detect(frame)
        return boxes, image_processing_batch(frame, boxes, self.image_options, centre_crop=True)

    def aligned_crops(self, image):
        """-> (list of BoundingBox, device uint8 [F, size, size, 3], Alignment): every detected face warped onto the five-point
        template by its own landmarks (`image_processing_aligned_batch`; a face that is not alignable keeps the box path's
        pixels).  With `max_residual`, aligned faces whose landmarks fit the template worse than that are dropped here, before
        any network launch."""
        frame = self._frame(image)
        boxes = self.detector.detect(frame)
        crops, alignment = image_processing_aligned_batch(frame, boxes, self.image_options)
        if self.max_residual is not None and len(boxes):
            keep = np.nonzero(~(alignment.residual > self.max_residual))[0]          # NaN (not aligned) stays
            if len(keep) < len(boxes):
                boxes, alignment = [boxes[i] for i in keep], alignment.take(keep)
                crops = crops[torch.from_numpy(keep).to(crops.device)]
        return boxes, crops, alignment

    def _batch(self, crops):
        """The crops zero-padded to the planned batch size that holds them."""
        batch = crops.new_zeros((padded_batch(crops.shape[0]),) + tuple(crops.shape[1:]))
        batch[:crops.shape[0]] = crops
        return batch

    def embed(self, crops):
        """device uint8 [F, size, size, 3] -> float32 [F, E] through FaceNet.evaluate at the padded batch size."""
        return np.asarray(self.facenet.evaluate(self._batch(crops)))[:crops.shape[0]]

    def faces(self, image):
        """-> list of (BoundingBox, float32 [E] embedding), [] without a network launch when nothing was detected."""
        boxes, crops = self.crops(image)
        if len(boxes) == 0:
            return []
        return list(zip(boxes, self.embed(crops)))

    def embed_device(self, crops):
        """`embed` without the copy to the host: device float32 [F, E] (a copy: the plan's output buffer is reused)."""
        return self.facenet.evaluate_device(self._batch(crops))[:crops.shape[0]].to(dtype=torch.float32, copy=True)

    def identify(self, image, gallery, **kw):
        """-> list of (BoundingBox, (label, name, distance, row)) through `gallery.identify(embeddings, **kw)`; [] without a
        network or search launch when nothing was detected.  The embeddings never visit the host."""
        boxes, crops = self.crops(image)
        if len(boxes) == 0:
            return []
        return list(zip(boxes, gallery.identify(self.embed_device(crops), **kw)))

    def identify_candidates(self, image, gallery, **kw):
        """-> list of (BoundingBox, [(label, name, distance, row), ...]) through `gallery.identify_candidates(embeddings, **kw)`:
        every face's candidate list of identities.  [] without a network or search launch when nothing was detected."""
        boxes, crops = self.crops(image)
        if len(boxes) == 0:
            return []
        return list(zip(boxes, gallery.identify_candidates(self.embed_device(crops), **kw)))

    def cluster(self, images, metric=0, method="dbscan", **kw):
        """Detect, crop and embed the faces of a list of photographs, then `Gallery.cluster(**kw)` them (``method='dbscan'``) or
        `Gallery.hdbscan(**kw)` them (``'hdbscan'``: no threshold); the embeddings never visit the host.
        -> (Clustering or HierarchicalClustering, faces): faces[row] = (image index, face index within the image, BoundingBox).
        Without a single face: (None, [])."""
        if method not in ("dbscan", "hdbscan"):
            raise ValueError(f"method must be 'dbscan' or 'hdbscan', got {method!r}")
        faces, embeddings = [], []
        for index, image in enumerate(images):
            boxes, crops = self.crops(image)
            if len(boxes) == 0:
                continue
            embeddings.append(self.embed_device(crops))
            faces.extend((index, n, box) for n, box in enumerate(boxes))
        if not faces:
            return None, []
        gallery = Gallery(torch.cat(embeddings), metric=metric, device=self.device)
        return (gallery.cluster(**kw) if method == "dbscan" else gallery.hdbscan(**kw)), faces
