"""From a photograph to the embeddings of the faces in it, on the device end to end.

``FacePipeline(detector, facenet, image_options)``: the frame is uploaded once; the same device tensor goes to the detector
(`FaceDetector.detect` -> MTCNN) and to the crop kernel (`image_processing_batch`, the pixels of `image_processing` followed by the
centre cut of `image.size`), whose uint8 output goes straight to `FaceNet.evaluate`.  The network plans one launch list (and
captures one graph) per batch size, so the face batch is zero-padded up to one of `BATCH_SIZES`: photos with 1, 2 or 3 faces
share a plan.  Inference has no coupling between the images of a batch, so the padding rows change nothing."""
from __future__ import annotations

import numpy as np
import torch

from .detectors.face_detector import image_processing_batch

BATCH_SIZES = (1, 4, 16, 64, 256)


def padded_batch(n: int) -> int:
    """The smallest planned batch size that holds n faces (multiples of the largest one beyond it)."""
    for size in BATCH_SIZES:
        if n <= size:
            return size
    return -(-n // BATCH_SIZES[-1]) * BATCH_SIZES[-1]


class FacePipeline:
    def __init__(self, detector, facenet, image_options, device="cuda:0"):
        self.detector, self.facenet, self.image_options = detector, facenet, image_options
        self.device = torch.device(device)

    def _frame(self, image):
        """uint8 [H, W, 3] in the detector's channel order -> the one device copy of it."""
        if torch.is_tensor(image):
            return image.to(device=self.device, dtype=torch.uint8).contiguous()
        arr = np.ascontiguousarray(np.asarray(image, dtype=np.uint8))
        return torch.from_numpy(arr if arr.flags.writeable else arr.copy()).to(self.device)

    def crops(self, image):
        """-> (list of BoundingBox, device uint8 [F, size, size, 3])."""
        frame = self._frame(image)
        boxes = self.detector.detect(frame)
        return boxes, image_processing_batch(frame, boxes, self.image_options, centre_crop=True)

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
