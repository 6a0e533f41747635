"""Mirror of facenet/detectors/face_detector.py (BoundingBox, image_processing, FaceDetector) with the 'pypimtcnn' detector
served by facenet_amd.detectors.mtcnn instead of the PyPI package.  The Faster-RCNN detector of the reference
(`detectors/frcnnv3`, a frozen TF1 graph whose weights are absent from the reference tree) is out of scope.

`image_processing_batch` is `image_processing` for all boxes of one frame on the device (`fn_face_crop_resize_u8`, DESIGN.md
section 17): the same pixels, bit for bit, without the frame or the thumbnails visiting the host."""
from __future__ import annotations

import math

import numpy as np
from PIL import Image

from . import mtcnn as _mtcnn


def image_processing(image, box, options):
    """face_detector.py:9-26: crop the box plus a relative margin, resize to size * (1 + margin) with PIL's antialias filter."""
    if not isinstance(image, Image.Image):
        raise ValueError('Input must be PIL.Image')
    dw, dh = round(box.width * options.margin / 2), round(box.height * options.margin / 2)
    side = math.ceil(options.size + options.size * options.margin)
    window = (box.left - dw, box.top - dh, box.right + dw, box.bottom + dh)
    return image.crop(window).resize((side, side), getattr(Image, "LANCZOS", None) or Image.ANTIALIAS)   # ANTIALIAS == LANCZOS


MAX_SIDE, MAX_EXTENT = 256, 3072      # FN_FACE_CROP_MAX_SIDE / FN_FACE_CROP_MAX_EXTENT of include/facenet_hip.h


def crop_table(boxes, options):
    """-> (int32 [F, 4] windows (left, top, right, bottom) with the margin added, side, centre offset): image_processing's own
    numbers for every box, and where the `options.size` centre cut of the side x side thumbnail starts."""
    side = math.ceil(options.size + options.size * options.margin)
    windows = np.empty((len(boxes), 4), np.int32)
    for i, box in enumerate(boxes):
        dw, dh = round(box.width * options.margin / 2), round(box.height * options.margin / 2)
        windows[i] = (box.left - dw, box.top - dh, box.right + dw, box.bottom + dh)
    return windows, side, (side - int(options.size)) // 2


def check_crop_arguments(windows, side, ox, oy, out_side):
    """The limits of fn_face_crop_resize_u8 as ValueError, before anything is launched."""
    windows = np.asarray(windows)
    if windows.ndim != 2 or windows.shape[1] != 4 or not 0 < windows.shape[0] <= 65535:
        raise ValueError(f"face crop: windows of shape {windows.shape}, [F, 4] with 1 <= F <= 65535 expected")
    if not 0 < side <= MAX_SIDE:
        raise ValueError(f"face crop: side {side} outside 1 .. {MAX_SIDE}")
    if out_side <= 0 or ox < 0 or oy < 0 or ox + out_side > side or oy + out_side > side:
        raise ValueError(f"face crop: output window ({ox}, {oy}) + {out_side} does not lie inside side {side}")
    extent = np.stack([windows[:, 2].astype(np.int64) - windows[:, 0], windows[:, 3].astype(np.int64) - windows[:, 1]])
    if extent.min() <= 0 or extent.max() > MAX_EXTENT:
        raise ValueError(f"face crop: windows of {extent.min()} .. {extent.max()} pixels per axis, 1 .. {MAX_EXTENT} expected")


_workspace = {}     # device -> int32 workspace of the tap tables, grown on demand


def crop_resize(frame, windows, side, ox=0, oy=0, out_side=None, stream=None):
    """`Image.fromarray(frame).crop(w).resize((side, side), LANCZOS)` for every window w -> device uint8 [F, S, S, 3]: rows / columns
    [oy, oy + S) x [ox, ox + S) of each result (S = out_side, the whole thumbnail by default).  frame: uint8 [H, W, 3], an array
    or a device tensor."""
    import ctypes as C

    import torch

    from .. import _lib
    out_side = side if out_side is None else out_side
    windows = np.ascontiguousarray(windows, dtype=np.int32)
    check_crop_arguments(windows, side, ox, oy, out_side)
    if not torch.is_tensor(frame):
        arr = np.ascontiguousarray(frame)
        frame = torch.from_numpy(arr if arr.flags.writeable else arr.copy()).to("cuda")
    if frame.dtype != torch.uint8 or frame.dim() != 3 or frame.shape[2] != 3 or not frame.is_cuda:
        raise ValueError("face crop: the frame must be uint8 [height, width, 3] (an array or a device tensor)")
    frame = frame.contiguous()
    lib = _lib.load()
    words = C.c_longlong(0)
    count = windows.shape[0]
    _lib.check(lib.fn_face_crop_workspace(windows.ctypes.data, count, side, C.byref(words)), "face_crop_workspace")
    work = _workspace.get(frame.device)
    if work is None or work.numel() < words.value:
        work = _workspace[frame.device] = torch.empty(words.value, dtype=torch.int32, device=frame.device)
    out = torch.empty(count, out_side, out_side, 3, dtype=torch.uint8, device=frame.device)
    with torch.cuda.device(frame.device):
        st = torch.cuda.current_stream().cuda_stream if stream is None else stream
        _lib.check(lib.fn_face_crop_resize_u8(frame.data_ptr(), frame.shape[0], frame.shape[1], windows.ctypes.data, count, side, ox, oy,
                                              out_side, out.data_ptr(), work.data_ptr(), work.numel(), st), "face_crop_resize")
    return out


def image_processing_batch(frame, boxes, options, centre_crop=False, stream=None):
    """`image_processing` for every box of one frame, on the device: uint8 [F, side, side, 3] holding the pixels of
    `image_processing(Image.fromarray(frame), box, options)`, or with centre_crop their [F, size, size, 3] centre (what
    resize_with_crop_or_pad(size) takes from them) without computing the border."""
    import torch
    windows, side, centre = crop_table(boxes, options)
    if len(boxes) == 0:
        out_side = int(options.size) if centre_crop else side
        device = frame.device if torch.is_tensor(frame) else "cuda"
        return torch.empty(0, out_side, out_side, 3, dtype=torch.uint8, device=device)
    if centre_crop:
        return crop_resize(frame, windows, side, centre, centre, int(options.size), stream)
    return crop_resize(frame, windows, side, stream=stream)


class BoundingBox:
    """face_detector.py:29-60: integer box with an exclusive right / bottom edge."""

    def __init__(self, left, top, width, height, confidence=None):
        self.left, self.top = int(np.round(left)), int(np.round(top))
        self.right, self.bottom = int(np.round(left + width)) + 1, int(np.round(top + height)) + 1
        self.width, self.height = self.right - self.left - 1, self.bottom - self.top - 1
        self.confidence = confidence

    def info(self, mode=False):
        fields = [self.left, self.top, self.width, self.height, self.confidence]
        if mode:
            return "left = {}, top = {}, width = {}, height = {}, confidence = {}".format(*fields)
        return str(fields)

    __repr__ = lambda self: self.info(mode=True)
    left_upper = property(lambda self: (self.left, self.top))
    right_lower = property(lambda self: (self.right, self.bottom))
    confidence_as_string = property(lambda self: str(np.round(self.confidence, 3)))


class MTCNN:
    """face_detector.py:63-78."""

    def __init__(self, **kwargs):
        self.__detector = _mtcnn.MTCNN(**kwargs).detect_faces
        self.mode = 'RGB'

    def detector(self, image):
        return [BoundingBox(left=f['box'][0], top=f['box'][1], width=f['box'][2], height=f['box'][3], confidence=f['confidence'])
                for f in self.__detector(image)]


class FaceDetector:
    """face_detector.py:98-123; `detector='pypimtcnn'` is the only one built (keyword arguments go to the MTCNN constructor)."""

    def __init__(self, detector='pypimtcnn', gpu_memory_fraction=1.0, **kwargs):
        if detector == 'frcnnv3':
            raise NotImplementedError("frcnnv3 (frozen Faster-RCNN graph, weights absent from the reference) is out of scope")
        if detector != 'pypimtcnn':
            raise ValueError('Undefined face detector type {}'.format(detector))
        backend = MTCNN(**kwargs)
        self.detector, self.mode, self._find = detector, backend.mode, backend.detector

    def detect(self, image):
        """image: uint8 array or device tensor [height, width, 3] in `self.mode` channel order -> list of BoundingBox."""
        return self._find(image)

    def __repr__(self):
        return f'class {type(self).__name__}\ndetector type: {self.detector}'
