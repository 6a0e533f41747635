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

``Gallery.mates`` is the search of the open-set evaluation: every probe's nearest mate, nearest impostor and
the rank of that mate at any depth, from fn_mate_search on the same walk and the same bits; ``statistics.IdentificationCurve``
turns them into FNIR at FPIR.

``Gallery.kmeans`` and ``Gallery.ivf`` (`ivf.py`): spherical k-means on the device and the inverted-file
index it trains; an `ivf.IVFGallery` searches only the lists a query probes, with `search`'s bits."""
from __future__ import annotations

import ctypes
from pathlib import Path
from typing import NamedTuple

import numpy as np
import torch

from . import _lib
from .detectors.face_detector import image_processing_aligned_batch, image_processing_batch
from .faceclass import _as_table, _ptr, _stream
from .statistics import check_unit_range

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

    def embed(self, crops):
        """device uint8 [F, size, size, 3] -> float32 [F, E] through FaceNet.evaluate at the padded batch size."""
        n = crops.shape[0]
        batch = crops.new_zeros((padded_batch(n),) + tuple(crops.shape[1:]))
        batch[:n] = crops
        return np.asarray(self.facenet.evaluate(batch))[:n]

    def faces(self, image):
        """-> list of (BoundingBox, float32 [E] embedding), [] without a network launch when nothing was detected."""
        boxes, crops = self.crops(image)
        if len(boxes) == 0:
            return []
        return list(zip(boxes, self.embed(crops)))

    def embed_device(self, crops):
        """`embed` without the copy to the host: device float32 [F, E] (a copy: the plan's output buffer is reused)."""
        n = crops.shape[0]
        batch = crops.new_zeros((padded_batch(n),) + tuple(crops.shape[1:]))
        batch[:n] = crops
        return self.facenet.evaluate_device(batch)[:n].to(dtype=torch.float32, copy=True)

    def identify(self, image, gallery, **kw):
        """-> list of (BoundingBox, (label, name, distance, row)) through `gallery.identify(embeddings, **kw)`; [] without a
        network or search launch when nothing was detected.  The embeddings never visit the host."""
        boxes, crops = self.crops(image)
        if len(boxes) == 0:
            return []
        return list(zip(boxes, gallery.identify(self.embed_device(crops), **kw)))

    def cluster(self, images, metric=0, **kw):
        """Detect, crop and embed the faces of a list of photographs, then `Gallery.cluster(**kw)` them; the embeddings never
        visit the host.  -> (Clustering, faces): faces[row] = (image index, face index within the image, BoundingBox).  Without a
        single face: (None, [])."""
        faces, embeddings = [], []
        for index, image in enumerate(images):
            boxes, crops = self.crops(image)
            if len(boxes) == 0:
                continue
            embeddings.append(self.embed_device(crops))
            faces.extend((index, n, box) for n, box in enumerate(boxes))
        if not faces:
            return None, []
        return Gallery(torch.cat(embeddings), metric=metric, device=self.device).cluster(**kw), faces


MAX_K = 64                # fn_gallery_search: 1 <= k <= 64
MAX_LENGTH = 512          # ... and embedding length a multiple of 4 up to 512


MAX_EDGES = 2 ** 31      # cols are int32 positions of a CSR that one allocation holds
DBSCAN_ROUNDS = 8         # rounds enqueued between two looks at the converged flag


def check_edges(nnz, max_edges=None):
    """The size rule of `Gallery.within`, applied before anything of that size is allocated."""
    if nnz >= MAX_EDGES:
        raise ValueError(f"the radius search found nnz = {nnz} neighbour pairs, 2^31 or more: choose a smaller eps")
    if max_edges is not None and nnz > max_edges:
        raise ValueError(f"the radius search found nnz = {nnz} neighbour pairs, more than max_edges = {max_edges}: choose a smaller eps")


class Clustering:
    """The result of `Gallery.cluster`: ``labels`` int64 [G] (cluster ids 0 .. nrof_clusters - 1 in ascending order of each
    cluster's smallest core row, -1 for noise), ``core`` bool [G], ``nrof_clusters``, ``nrof_noise``, ``rounds`` (hook-and-jump
    rounds run), ``eps`` / ``min_samples`` and the CSR it was built from: ``offsets`` int64 [G + 1], ``rows`` int32 [nnz],
    ``dist`` float32 [nnz] (device tensors)."""

    def __init__(self, labels, core, nrof_clusters, nrof_noise, rounds, eps, min_samples, offsets, rows, dist):
        self.labels, self.core = labels, core
        self.nrof_clusters, self.nrof_noise, self.rounds = nrof_clusters, nrof_noise, rounds
        self.eps, self.min_samples = eps, min_samples
        self.offsets, self.rows, self.dist = offsets, rows, dist

    @property
    def sizes(self):
        """int64 [nrof_clusters]: rows per cluster (noise rows are in none)."""
        return np.bincount(self.labels[self.labels >= 0], minlength=self.nrof_clusters).astype(np.int64)

    def members(self, c):
        """The rows of cluster c, ascending (c = -1: the noise rows)."""
        if not -1 <= c < self.nrof_clusters:
            raise ValueError(f"cluster {c} is not in [-1, {self.nrof_clusters})")
        return np.nonzero(self.labels == c)[0]

    def __repr__(self):
        return (f"{self.__class__.__name__}\n" + f"Number of images {len(self.labels)}\n" + f"Number of clusters {self.nrof_clusters}\n" +
                f"Number of noise images {self.nrof_noise}\n" + f"eps: {self.eps} min_samples: {self.min_samples}\n")


class MateSearch(NamedTuple):
    """What `Gallery.mates` returns, one entry per query row: the nearest mate's distance (float32) and gallery row (int32), the
    nearest impostor's, and ``ranks`` int32 (None when not asked for): the impostor rows nearer than the nearest mate.  Row -1,
    distance +inf and rank -1 where there is no such row."""
    mate_dist: object
    mate_rows: object
    impostor_dist: object
    impostor_rows: object
    ranks: object


def _class_names(labels, files):
    """label -> the name of the directory that holds one of its files (the class directories of dataset.Database)."""
    names = {}
    for label, f in zip(np.asarray(labels).tolist(), np.asarray(files).tolist()):
        names.setdefault(int(label), Path(str(f)).parent.name)
    return names


class Gallery:
    """The known faces: fp32 unit-norm embeddings [G, E] resident on the device, optionally an integer label per row (default:
    every row is its own class), a name per label (a dict, or a sequence indexed by label) and the file of every row.  ``metric``
    0 reports 2 (1 - x.y), 1 arccos(x.y) (statistics.py:45-53); both rank by the former.  Labels stay on the host as int64 and
    are looked up there from the rows a search returns (fn_gallery_search's own int32 ``labels`` table is not used), so any
    non-negative integer is a valid label."""

    def __init__(self, embeddings, labels=None, names=None, files=None, metric=0, device="cuda"):
        if metric not in (0, 1):
            raise ValueError("Undefined similarity metric {}".format(metric))            # statistics.py:55
        shape = tuple(embeddings.shape) if hasattr(embeddings, "shape") else np.shape(embeddings)
        if len(shape) != 2 or shape[0] < 1:
            raise ValueError(f"gallery embeddings must be a non-empty 2-D [G, E] array, got shape {shape}")
        if shape[1] % 4 or not 4 <= shape[1] <= MAX_LENGTH:
            raise ValueError(f"embedding length {shape[1]} must be a multiple of 4 in [4, {MAX_LENGTH}]")
        if labels is None:
            host_labels = np.arange(shape[0], dtype=np.int64)
        else:
            host_labels = np.asarray(labels.cpu() if torch.is_tensor(labels) else labels)
            if host_labels.shape != (shape[0],) or host_labels.dtype.kind not in "iu":
                raise ValueError(f"labels must be {shape[0]} integers, got shape {host_labels.shape} of {host_labels.dtype}")
            if host_labels.min() < 0:
                raise ValueError("labels must not be negative: -1 is what an unidentified face gets")
        if files is not None and len(files) != shape[0]:
            raise ValueError(f"files must name {shape[0]} rows, got {len(files)}")
        if names is not None and not isinstance(names, dict):
            names = {i: n for i, n in enumerate(names)}
        if names is not None and not set(np.unique(host_labels).tolist()) <= set(names):
            raise ValueError("names must cover every label")
        self.metric, self.device = metric, torch.device(device)
        self.labels = host_labels.astype(np.int64)
        self.names = names
        self.files = None if files is None else np.asarray(files, dtype=str)
        self.embeddings = _as_table(embeddings, self.device)
        self._codes = None         # `_label_codes`

    @classmethod
    def from_file(cls, path, metric=0, device="cuda"):
        """The .npz of apps/embeddings.py (``embeddings`` / ``labels`` / ``files``); names are the class directories of ``files``."""
        path = Path(path).expanduser()
        if path.suffix == ".h5":
            raise ValueError(f"{path}: .h5 embeddings files need h5py, which this project does not use; "
                             "write an .npz with 'embeddings' and 'labels' (facenet_amd.apps.embeddings)")
        with np.load(path) as f:
            embeddings = np.asarray(f["embeddings"], dtype=np.float32)
            labels = np.asarray(f["labels"]) if "labels" in f else None
            files = np.asarray(f["files"]) if "files" in f else None
        names = _class_names(labels, files) if labels is not None and files is not None else None
        return cls(embeddings, labels=labels, names=names, files=files, metric=metric, device=device)

    @property
    def nrof_images(self):
        return self.embeddings.shape[0]

    @property
    def nrof_classes(self):
        return len(np.unique(self.labels))

    @property
    def length(self):
        return self.embeddings.shape[1]

    def __repr__(self):
        return (f"{self.__class__.__name__}\n" + f"Number of classes {self.nrof_classes} \n" + f"Number of images {self.nrof_images}\n" +
                f"Embedding length {self.length}\n" + f"metric: {self.metric}\n")

    def _queries(self, queries, skip, runs):
        """The checks `search` and `within` share -> (Q, the queries as a device table, the int32 skip tensor or None); for
        Q = 0 the last two are None, and nothing needs a device.  ``runs``: what the caller runs, for the error without one."""
        shape = tuple(queries.shape) if hasattr(queries, "shape") else np.shape(queries)
        if len(shape) != 2:
            raise ValueError(f"queries must be a 2-D [Q, E] array, got shape {shape}")
        if shape[1] != self.length:
            raise ValueError(f"embedding lengths differ: queries {shape[1]}, gallery {self.length}")
        Q = shape[0]
        if skip is not None:
            skip = np.asarray(skip.cpu() if torch.is_tensor(skip) else skip)
            if skip.shape != (Q,) or skip.dtype.kind not in "iu":
                raise ValueError(f"skip must be {Q} integers (a gallery row, or -1), got shape {skip.shape} of {skip.dtype}")
        if Q == 0:
            return 0, None, None
        if self.device.type != "cuda":
            raise _lib.FacenetHipError(f"{runs} on the GPU; facenet_amd has no CPU fallback")
        skip_dev = None if skip is None else torch.from_numpy(skip.astype(np.int32)).to(self.device)
        return Q, _as_table(queries, self.device), skip_dev

    def _workspace(self, sizer, what, *args):
        """The int64 workspace tensor of the size that sizer(*args, &bytes), a fn_*_workspace entry, reports (at least 8 bytes)."""
        nbytes = ctypes.c_longlong(0)
        _lib.check(sizer(*args, ctypes.byref(nbytes)), what)
        return torch.empty(max(1, (nbytes.value + 7) // 8), dtype=torch.int64, device=self.device)

    def _search(self, queries, k, skip, slab_rows, atol):
        """-> device (dist [Q, k], rows [Q, k]) after every check of `search`."""
        k = int(k)
        if not 1 <= k <= MAX_K:
            raise ValueError(f"k must be in [1, {MAX_K}], got {k}")
        Q, q, skip_dev = self._queries(queries, skip, "Gallery.search runs fn_gallery_search")
        dev, G = self.device, self.nrof_images
        dist = torch.empty((Q, k), dtype=torch.float32, device=dev)
        rows = torch.empty((Q, k), dtype=torch.int32, device=dev)
        if Q == 0:
            return dist, rows
        lib = _lib.load()
        ws = self._workspace(lib.fn_gallery_search_workspace, "gallery_search_workspace", Q, G, k, int(slab_rows))
        rng = None if atol is None else torch.zeros(2, dtype=torch.int32, device=dev)
        _lib.check(lib.fn_gallery_search(_ptr(q), Q, _ptr(self.embeddings), G, self.length, k, self.metric, _ptr(skip_dev), None, int(slab_rows),
                                         _ptr(ws), _ptr(dist), _ptr(rows), None, _ptr(rng), _stream(dev)),
                   "gallery_search")
        if rng is not None:
            check_unit_range(rng, atol)         # waits for the search
        return dist, rows

    def search(self, queries, k=1, skip=None, slab_rows=0, atol=1.e-5):
        """The k nearest gallery rows of every query row -> (dist float32 [Q, k], rows int32 [Q, k]), ascending by (distance,
        row); NumPy in gives NumPy out, a device tensor in gives device tensors out.  ``skip`` [Q]: the gallery row query q must
        not return (-1: none).  A query with fewer than k admissible rows gets row -1 at distance +inf in the tail.  Raises the
        reference's ValueError when some dot product leaves +-(1 + atol); that check reads two words back and so waits for the
        search on the host, also when tensors go in and come out.  ``atol=None`` leaves the check out: the call then only
        enqueues work on the current stream.  ``slab_rows`` is fn_gallery_search's (0: chosen by the library; the result does not
        depend on it)."""
        dist, rows = self._search(queries, k, skip, slab_rows, atol)
        if torch.is_tensor(queries):
            return dist, rows
        return dist.cpu().numpy(), rows.cpu().numpy()

    def leave_one_out(self, k=1):
        """Every gallery row's k nearest OTHER rows, device tensors: ``search(gallery, k, skip=arange(G))``."""
        return self.search(self.embeddings, k, skip=np.arange(self.nrof_images, dtype=np.int32))

    def kmeans(self, nlist, iters=10, seed=0):
        """Spherical k-means of the gallery's rows into ``nlist`` groups on the device -> (centroids fp32
        [nlist, E], assign int32 [G], info): `ivf.kmeans`.  Reproducible bit for bit for a given seed."""
        from .ivf import kmeans
        return kmeans(self, nlist, iters, seed)

    def ivf(self, nlist, iters=10, seed=0):
        """The inverted-file index of this gallery over the k-means of its rows -> `ivf.IVFGallery`, whose searches walk only
        the lists a query probes."""
        from .ivf import ivf
        return ivf(self, nlist, iters, seed)

    def _label_codes(self):
        """(the gallery's sorted unique labels int64 [C], device int32 [G] dense codes 0 .. C - 1), built once: fn_mate_search
        compares int32 codes, whatever non-negative int64 the labels are."""
        if self._codes is None:
            uniq, inverse = np.unique(self.labels, return_inverse=True)
            codes = torch.from_numpy(inverse.reshape(-1).astype(np.int32))
            self._codes = (uniq, codes.to(self.device) if self.device.type == "cuda" else codes)
        return self._codes

    def query_codes(self, labels, Q):
        """Query labels -> int32 [Q] codes of the gallery's table: -1 for -1 and for a label the gallery does not hold."""
        labels = np.asarray(labels.cpu() if torch.is_tensor(labels) else labels)
        if labels.shape != (Q,) or (Q and labels.dtype.kind not in "iu"):        # (an empty list has no integer type)
            raise ValueError(f"labels must be {Q} integers (the probe's identity, or -1), got shape {labels.shape} of {labels.dtype}")
        labels = labels.astype(np.int64)
        if Q and labels.min() < -1:
            raise ValueError("a query label must not be below -1: -1 is a probe known to be absent from the gallery")
        uniq = self._label_codes()[0]
        at = np.minimum(np.searchsorted(uniq, labels), len(uniq) - 1)
        return np.where(uniq[at] == labels, at, -1).astype(np.int32)

    def _mates(self, queries, labels, skip, ranks, slab_rows, atol):
        """-> device (dist float32 [Q, 2], rows int32 [Q, 2], ranks int32 [Q] or None) after every check of `mates`."""
        shape = tuple(queries.shape) if hasattr(queries, "shape") else np.shape(queries)
        if len(shape) == 2 and shape[1] == self.length:        # (else `_queries` raises)
            codes = self.query_codes(labels, shape[0])         # before anything needs a device
        Q, q, skip_dev = self._queries(queries, skip, "Gallery.mates runs fn_mate_search")
        dev, G = self.device, self.nrof_images
        dist = torch.empty((Q, 2), dtype=torch.float32, device=dev)
        rows = torch.empty((Q, 2), dtype=torch.int32, device=dev)
        rank = torch.empty(Q, dtype=torch.int32, device=dev) if ranks else None
        if Q == 0:
            return dist, rows, rank
        lib = _lib.load()
        ws = self._workspace(lib.fn_mate_search_workspace, "mate_search_workspace", Q, G, int(slab_rows))
        rng = None if atol is None else torch.zeros(2, dtype=torch.int32, device=dev)
        qcodes = torch.from_numpy(codes).to(dev)
        _lib.check(lib.fn_mate_search(_ptr(q), Q, _ptr(qcodes), _ptr(self.embeddings), G, _ptr(self._label_codes()[1]), self.length, self.metric,
                                      _ptr(skip_dev), int(slab_rows), _ptr(ws), _ptr(dist), _ptr(rows), _ptr(rank), _ptr(rng), _stream(dev)),
                   "mate_search")
        if rng is not None:
            check_unit_range(rng, atol)         # waits for the search
        return dist, rows, rank

    def mates(self, queries, labels, skip=None, ranks=True, slab_rows=0, atol=1.e-5):
        """The open-set evaluation search: for every query row its nearest MATE (the nearest gallery row
        that carries the query's label) and its nearest IMPOSTOR (the nearest row of any other label) -> `MateSearch`; NumPy in
        gives NumPy out, a device tensor in gives device tensors out.  ``labels`` [Q]: the probes' identities in the gallery's
        own labels; -1, or a label the gallery does not hold, is a probe without a mate: every row is its impostor.  ``ranks``:
        also the number of impostor rows nearer than the nearest mate (-1 without a mate), the 0-based rank of the first mate in
        the full ordering, at any depth; it costs a second walk of the gallery.  Where there is no such row: row -1, distance
        +inf.  Equal distances go to the lower row; the distances are `search`'s bit for bit.  ``skip``, ``slab_rows``,
        ``atol``: as `search`."""
        dist, rows, rank = self._mates(queries, labels, skip, ranks, slab_rows, atol)
        out = (dist[:, 0], rows[:, 0], dist[:, 1], rows[:, 1], rank)
        if not torch.is_tensor(queries):
            out = tuple(None if t is None else t.cpu().numpy() for t in out)
        return MateSearch(*out)

    def leave_one_out_mates(self, ranks=True):
        """Every gallery row as a probe against all OTHER rows, device tensors: ``mates(gallery, labels, skip=arange(G))``."""
        return self.mates(self.embeddings, self.labels, skip=np.arange(self.nrof_images, dtype=np.int32), ranks=ranks)

    def threshold_of(self, threshold=None, classifier=None):
        """The fp32 threshold of `identify`: the number given, a classifier's trained one, or None (closed set)."""
        if threshold is not None and classifier is not None:
            raise ValueError("identify takes a threshold or a classifier, not both")
        if classifier is not None:
            from .faceclass import FaceToFaceNormalizedEmbeddingsClassifier
            if not isinstance(classifier, FaceToFaceNormalizedEmbeddingsClassifier):
                raise ValueError("identify needs a FaceToFaceNormalizedEmbeddingsClassifier: its distance is the gallery's metric 0")
            if self.metric != 0:
                raise ValueError("a classifier's threshold applies to metric 0, this gallery reports metric {}".format(self.metric))
            return classifier.variable("threshold", mode="numpy")
        return None if threshold is None else np.float32(threshold)

    def identify(self, queries, threshold=None, classifier=None, k=1):
        """-> for every query row (label, name, distance, row) of its nearest gallery row.  ``k`` is the width of the search that
        is run; only its best column is used, so any k gives the same answer and k = 1 is the cheapest.  Open set:
        label -1 and name None unless ``distance < threshold`` (the strict < of the classifiers' predict, in fp32); the
        threshold is the number given or ``classifier.variable("threshold")``.  Neither: closed set, always the nearest."""
        thr = self.threshold_of(threshold, classifier)
        dist, rows = self._search(queries, k, None, 0, 1.e-5)
        return [self.who(d, r, thr) for d, r in zip(dist[:, 0].cpu().numpy(), rows[:, 0].cpu().numpy())]

    def who(self, distance, row, threshold=None):
        """(label, name, distance, row) of one search result: label -1, name None when there is no row or, with an fp32
        ``threshold`` (`threshold_of`), ``distance < threshold`` is false."""
        known = row >= 0 and (threshold is None or distance < threshold)
        label = int(self.labels[row]) if known else -1
        return label, (self.names[label] if known and self.names is not None else None), float(distance), int(row)

    def _within(self, queries, eps, skip, slab_rows, atol, max_edges):
        """-> device (offsets int64 [Q + 1], rows int32 [nnz], dist float32 [nnz]) after every check of `within`."""
        eps = np.float32(eps)
        if np.isnan(eps):
            raise ValueError("eps must be a number, got NaN")
        if max_edges is not None and max_edges < 0:
            raise ValueError(f"max_edges must not be negative, got {max_edges}")
        Q, q, skip_dev = self._queries(queries, skip, "Gallery.within runs fn_radius_count")
        dev, G = self.device, self.nrof_images
        offsets = torch.zeros(Q + 1, dtype=torch.int64, device=dev)
        if Q == 0:
            return offsets, torch.empty(0, dtype=torch.int32, device=dev), torch.empty(0, dtype=torch.float32, device=dev)
        lib = _lib.load()
        ws = self._workspace(lib.fn_radius_workspace, "radius_workspace", Q, G, int(slab_rows))
        rng = torch.zeros(2, dtype=torch.int32, device=dev)
        common = (_ptr(q), Q, _ptr(self.embeddings), G, self.length, self.metric, float(eps), _ptr(skip_dev), int(slab_rows), _ptr(ws))
        _lib.check(lib.fn_radius_count(*common, _ptr(offsets), _ptr(rng), _stream(dev)), "radius_count")
        nnz = int(offsets[Q].item())                                # waits for the count
        if atol is not None:
            check_unit_range(rng, atol)
        check_edges(nnz, max_edges)
        rows = torch.empty(nnz, dtype=torch.int32, device=dev)
        dist = torch.empty(nnz, dtype=torch.float32, device=dev)
        if nnz:
            _lib.check(lib.fn_radius_fill(*common, _ptr(rows), _ptr(dist), nnz, _stream(dev)), "radius_fill")
        return offsets, rows, dist

    def within(self, queries, eps, skip=None, slab_rows=0, atol=1.e-5, max_edges=None):
        """Every gallery row at ``distance < eps`` (the gallery's metric, strict fp32 <) of every query row, as a CSR ->
        (offsets int64 [Q + 1], rows int32 [nnz], dist float32 [nnz]): query q's neighbours are rows[offsets[q]:offsets[q + 1]],
        ascending by gallery row.  NumPy in gives NumPy out, a device tensor in gives device tensors out.  ``skip`` [Q]: the
        gallery row query q must not return (-1: none).  The call reads nnz back between its two passes, so it waits for the
        device.  Raises the reference's ValueError when some dot product leaves +-(1 + atol) (``atol=None``: no such check), and a
        ValueError naming nnz when it exceeds ``max_edges`` or reaches 2^31, before the rows are allocated.  ``slab_rows`` is
        fn_radius_count's (0: chosen by the library; the result does not depend on it)."""
        out = self._within(queries, eps, skip, slab_rows, atol, max_edges)
        if torch.is_tensor(queries):
            return out
        return tuple(t.cpu().numpy() for t in out)

    def neighbours(self, eps, max_edges=None):
        """The self-join, device tensors: every gallery row's OTHER rows within eps, ``within(gallery, eps, skip=arange(G))``.
        The distances are symmetric bit for bit, so row j is in i's list exactly when i is in j's."""
        return self.within(self.embeddings, eps, skip=np.arange(self.nrof_images, dtype=np.int32), max_edges=max_edges)

    def cluster(self, threshold=None, classifier=None, min_samples=1, max_edges=None):
        """DBSCAN over the gallery's rows at eps = the threshold (a number, or a trained classifier's: `threshold_of`) -> a
        `Clustering`.  A row is a core row when it has at least ``min_samples`` rows within eps, itself included; clusters are
        the connected components of the core rows; a non-core row with a core neighbour joins its nearest core neighbour's
        cluster (equal distances: the lower row); every other row is noise, label -1.  ``min_samples=1`` is single linkage at
        the threshold."""
        if threshold is None and classifier is None:
            raise ValueError("cluster needs a threshold or a classifier: clustering has no closed set")
        if isinstance(min_samples, bool) or not isinstance(min_samples, (int, np.integer)) or min_samples < 1:
            raise ValueError(f"min_samples must be an integer of at least 1, got {min_samples!r}")
        eps = self.threshold_of(threshold, classifier)
        offsets, rows, dist = self.neighbours(eps, max_edges=max_edges)
        dev, N = self.device, self.nrof_images
        lib = _lib.load()
        labels = torch.empty(N, dtype=torch.int32, device=dev)
        core = torch.empty(N, dtype=torch.int32, device=dev)
        ids = torch.empty(N, dtype=torch.int32, device=dev)
        info = torch.zeros(8, dtype=torch.int32, device=dev)
        st = _stream(dev)
        _lib.check(lib.fn_dbscan_init(N, _ptr(offsets), int(min_samples), _ptr(labels), _ptr(core), _ptr(info), st), "dbscan_init")
        while True:
            _lib.check(lib.fn_dbscan_rounds(N, _ptr(offsets), _ptr(rows), _ptr(core), _ptr(labels), _ptr(info), DBSCAN_ROUNDS, st), "dbscan_rounds")
            if int(info[0].item()):
                break
        _lib.check(lib.fn_dbscan_finish(N, _ptr(offsets), _ptr(rows), _ptr(dist), self.metric, _ptr(self.embeddings), self.length, _ptr(core),
                                        _ptr(labels), _ptr(ids), _ptr(info), st), "dbscan_finish")
        _, rounds, clusters, noise = info.cpu().tolist()[:4]
        return Clustering(labels.cpu().numpy().astype(np.int64), core.cpu().numpy().astype(bool), clusters, noise, rounds, float(eps),
                          int(min_samples), offsets, rows, dist)
