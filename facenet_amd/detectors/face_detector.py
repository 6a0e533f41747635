"""Mirror of facenet/detectors/face_detector.py (BoundingBox, image_processing, FaceDetector) with the 'pypimtcnn' detector
served by facenet_amd.detectors.mtcnn instead of the PyPI package.  The Faster-RCNN detector of the reference
(`detectors/frcnnv3`, a frozen TF1 graph whose weights are absent from the reference tree) is out of scope.

`image_processing_batch` is `image_processing` for all boxes of one frame on the device (`fn_face_crop_resize_u8`, DESIGN.md
section 17): the same pixels, bit for bit, without the frame or the thumbnails visiting the host.

`image_processing_aligned_batch` is the optional landmark alignment: a least-squares similarity from the
detector's five landmarks onto the ArcFace template (`similarity_from_landmarks`, host arithmetic) and one warp launch for all
faces of the frame (`align_faces` -> `fn_face_align_u8`); boxes without usable landmarks keep the box path's pixels."""
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


def _device_frame(frame, what):
    """uint8 [H, W, 3], an array or a device tensor -> the contiguous device tensor (an array is uploaded)."""
    import torch
    if not torch.is_tensor(frame):
        arr = np.ascontiguousarray(frame)
        frame = torch.from_numpy(arr if arr.flags.writeable else arr.copy()).to("cuda")
    if frame.dtype != torch.uint8 or frame.dim() != 3 or frame.shape[2] != 3 or not frame.is_cuda:
        raise ValueError(f"{what}: the frame must be uint8 [height, width, 3] (an array or a device tensor)")
    return frame.contiguous()


def crop_resize(frame, windows, side, ox=0, oy=0, out_side=None, stream=None):
    """`Image.fromarray(frame).crop(w).resize((side, side), LANCZOS)` for every window w -> device uint8 [F, S, S, 3]: rows / columns
    [oy, oy + S) x [ox, ox + S) of each result (S = out_side, the whole thumbnail by default).  frame: uint8 [H, W, 3], an array
    or a device tensor."""
    import torch

    from .. import _call, _lib
    out_side = side if out_side is None else out_side
    windows = np.ascontiguousarray(windows, dtype=np.int32)
    check_crop_arguments(windows, side, ox, oy, out_side)
    frame = _device_frame(frame, "face crop")
    lib = _lib.load()
    count = windows.shape[0]
    words = _call.workspace_size(lib.fn_face_crop_workspace, "face_crop_workspace", windows.ctypes.data, count, side)
    work = _workspace.get(frame.device)
    if work is None or work.numel() < words:
        work = _workspace[frame.device] = torch.empty(words, dtype=torch.int32, device=frame.device)
    out = torch.empty(count, out_side, out_side, 3, dtype=torch.uint8, device=frame.device)
    with torch.cuda.device(frame.device):
        st = _call.stream() if stream is None else stream
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


# ---- landmark alignment (the definition is restated in tests/align_oracle.py) ---------------------------
# the published five-point template of a 112 x 112 face, pixel-index coordinates, in MTCNN's landmark order
ARCFACE_112 = ((38.2946, 51.6963), (73.5318, 51.5014), (56.0252, 71.7366), (41.5493, 92.3655), (70.7299, 92.2041))
ALIGN_MAX_SIDE, ALIGN_MAX_SAMPLES = 256, 8     # FN_FACE_ALIGN_MAX_SIDE / FN_FACE_ALIGN_MAX_SAMPLES of include/facenet_hip.h
ALIGN_MAX_ENTRY = float(1 << 24)               # every entry of an inverse transform stays below this in magnitude
ALIGN_SIGMA = (1 / 16, 32.0)                   # source pixels per output pixel of an alignable face


def align_template(size, margin=0):
    """The template for a size x size output, float64 [5, 2] (x, y): the pixel centres of ARCFACE_112 scaled about the image
    centre; `margin` (the `image.margin` of the box path) shrinks the face by 1 / (1 + margin)."""
    return (np.asarray(ARCFACE_112, np.float64) + 0.5 - 56) * (size / 112) / (1 + margin) + size / 2 - 0.5


class Alignment:
    """The fitted transforms of F faces: ``inverse`` float64 [F, 6] (output pixel -> frame, rows (i0, i1, i2), (i3, i4, i5)),
    ``samples`` int32 [F] (sub-samples per axis of the box prefilter), ``ok`` bool [F] (alignable), and per face the roll
    ``angle`` in degrees, the ``scale`` from frame to output and the rms ``residual`` of the fit relative to the output size.
    A face that is not alignable has NaN everywhere and 0 samples."""

    def __init__(self, inverse, samples, ok, angle, scale, residual):
        self.inverse, self.samples, self.ok = inverse, samples, ok
        self.angle, self.scale, self.residual = angle, scale, residual

    def __len__(self):
        return len(self.ok)

    def take(self, rows):
        """The Alignment of a subset of the faces."""
        return Alignment(np.ascontiguousarray(self.inverse[rows]), np.ascontiguousarray(self.samples[rows]), self.ok[rows], self.angle[rows],
                         self.scale[rows], self.residual[rows])


def align_samples(sigma):
    """Sub-samples per axis of the box prefilter for `sigma` source pixels per output pixel: min(8, max(1, ceil(sigma)))."""
    return np.clip(np.ceil(sigma), 1, ALIGN_MAX_SAMPLES).astype(np.int32)


def _sum5(t):
    """Left-to-right sum over the five landmarks of [F, 5] (the order of the definition)."""
    return t[:, 0] + t[:, 1] + t[:, 2] + t[:, 3] + t[:, 4]


def similarity_from_landmarks(landmarks, template, size=112):
    """The least-squares proper similarity (rotation, uniform scale, translation; never a reflection) from each face's frame
    landmarks [F, 5, 2] onto `template` [5, 2], in closed form and float64 -> Alignment.  `size` is the output side the template
    was made for; only the residual uses it.  A face is alignable when its ten numbers are finite, its points do not coincide,
    it takes 1/16 .. 32 source pixels per output pixel and every inverse entry stays below 2^24; the others get ok = False."""
    p = np.asarray(landmarks, np.float64).reshape(-1, 5, 2)
    q = np.asarray(template, np.float64).reshape(5, 2)
    with np.errstate(all="ignore"):
        px, py, qx, qy = p[:, :, 0], p[:, :, 1], q[None, :, 0], q[None, :, 1]
        pmx, pmy, qmx, qmy = _sum5(px) / 5, _sum5(py) / 5, _sum5(qx) / 5, _sum5(qy) / 5
        cx, cy, dx, dy = px - pmx[:, None], py - pmy[:, None], qx - qmx[:, None], qy - qmy[:, None]
        den = _sum5(cx * cx + cy * cy)
        a, b = _sum5(cx * dx + cy * dy) / den, _sum5(cx * dy - cy * dx) / den
        tx, ty = qmx - (a * pmx - b * pmy), qmy - (b * pmx + a * pmy)
        d = a * a + b * b
        ia, ib = a / d, -b / d
        inverse = np.stack([ia, -ib, -(ia * tx - ib * ty), ib, ia, -(ib * tx + ia * ty)], axis=1)
        sigma = 1 / np.sqrt(d)
        ex, ey = (a[:, None] * px - b[:, None] * py) + tx[:, None] - qx, (b[:, None] * px + a[:, None] * py) + ty[:, None] - qy
        residual = np.sqrt(_sum5(ex * ex + ey * ey) / 5) / size
        ok = (np.isfinite(p).all(axis=(1, 2)) & np.isfinite(den) & (den > 0) & np.isfinite(d) & (d > 0) &
              (sigma >= ALIGN_SIGMA[0]) & (sigma <= ALIGN_SIGMA[1]) & (np.abs(inverse) < ALIGN_MAX_ENTRY).all(axis=1))
        samples = np.where(ok, align_samples(np.where(ok, sigma, 1.0)), 0).astype(np.int32)
        return Alignment(np.where(ok[:, None], inverse, np.nan), samples, ok, np.where(ok, np.degrees(np.arctan2(b, a)), np.nan),
                         np.where(ok, np.sqrt(d), np.nan), np.where(ok, residual, np.nan))


def check_align_arguments(inverse, samples, size):
    """The limits of fn_face_align_u8 as ValueError, before anything is launched."""
    inverse, samples = np.asarray(inverse), np.asarray(samples)
    if inverse.ndim != 2 or inverse.shape[1] != 6 or not 0 < inverse.shape[0] <= 65535:
        raise ValueError(f"face align: transforms of shape {inverse.shape}, [F, 6] with 1 <= F <= 65535 expected")
    if samples.shape != (inverse.shape[0],):
        raise ValueError(f"face align: samples of shape {samples.shape} for {inverse.shape[0]} faces")
    if not 0 < size <= ALIGN_MAX_SIDE:
        raise ValueError(f"face align: size {size} outside 1 .. {ALIGN_MAX_SIDE}")
    if samples.min() < 1 or samples.max() > ALIGN_MAX_SAMPLES:
        raise ValueError(f"face align: {samples.min()} .. {samples.max()} sub-samples per axis, 1 .. {ALIGN_MAX_SAMPLES} expected "
                         "(0 marks a face that is not alignable)")
    if not (np.abs(inverse) < ALIGN_MAX_ENTRY).all():        # a NaN fails the comparison too
        raise ValueError("face align: every inverse entry must be finite and below 2^24 in magnitude (NaN marks a face that is not alignable)")


_align_workspace = {}     # device -> int64 workspace of the transform tables, grown on demand


def align_faces(frame, alignment, size, stream=None):
    """Warp every face of `alignment` (all of them alignable) out of the frame -> device uint8 [F, size, size, 3], one
    fn_face_align_u8 launch.  frame: uint8 [H, W, 3], an array or a device tensor."""
    import torch

    from .. import _call, _lib
    inverse = np.ascontiguousarray(alignment.inverse, dtype=np.float64)
    samples = np.ascontiguousarray(alignment.samples, dtype=np.int32)
    size = int(size)
    check_align_arguments(inverse, samples, size)
    frame = _device_frame(frame, "face align")
    lib = _lib.load()
    count = inverse.shape[0]
    nbytes = _call.workspace_size(lib.fn_face_align_workspace, "face_align_workspace", count)
    work = _align_workspace.get(frame.device)
    if work is None or work.numel() * 8 < nbytes:
        work = _align_workspace[frame.device] = torch.empty(nbytes // 8, dtype=torch.int64, device=frame.device)
    out = torch.empty(count, size, size, 3, dtype=torch.uint8, device=frame.device)
    with torch.cuda.device(frame.device):
        st = _call.stream() if stream is None else stream
        _lib.check(lib.fn_face_align_u8(frame.data_ptr(), frame.shape[0], frame.shape[1], inverse.ctypes.data, samples.ctypes.data, count, size,
                                        out.data_ptr(), work.data_ptr(), work.numel() * 8, st), "face_align")
    return out


def image_processing_aligned_batch(frame, boxes, options, stream=None):
    """The network's input for every box of one frame, aligned where that is possible -> (device uint8 [F, size, size, 3],
    Alignment).  A box whose `landmarks` are alignable is warped onto `align_template(options.size, options.margin)`; every
    other row holds the bytes of `image_processing_batch(frame, [box], options, centre_crop=True)`."""
    import torch
    size = int(options.size)
    points = np.full((len(boxes), 5, 2), np.nan)
    for i, box in enumerate(boxes):
        if getattr(box, "landmarks", None) is not None:
            points[i] = box.landmarks
    alignment = similarity_from_landmarks(points, align_template(size, options.margin), size)
    if len(boxes) == 0:
        return image_processing_batch(frame, boxes, options, centre_crop=True), alignment
    frame = _device_frame(frame, "face align")         # one upload for both routes
    aligned, boxed = np.nonzero(alignment.ok)[0], np.nonzero(~alignment.ok)[0]
    if len(boxed) == 0:
        return align_faces(frame, alignment, size, stream), alignment
    out = torch.empty(len(boxes), size, size, 3, dtype=torch.uint8, device=frame.device)
    out[torch.from_numpy(boxed).to(frame.device)] = image_processing_batch(frame, [boxes[i] for i in boxed], options, centre_crop=True, stream=stream)
    if len(aligned):
        out[torch.from_numpy(aligned).to(frame.device)] = align_faces(frame, alignment.take(aligned), size, stream)
    return out, alignment


class BoundingBox:
    """face_detector.py:29-60: integer box with an exclusive right / bottom edge.  `landmarks`: the detector's five points in
    frame coordinates, float32 [5, 2] (x, y) in the order left eye, right eye, nose, mouth left, mouth right, or None."""

    def __init__(self, left, top, width, height, confidence=None, landmarks=None):
        self.left, self.top = int(np.round(left)), int(np.round(top))
        self.right, self.bottom = int(np.round(left + width)) + 1, int(np.round(top + height)) + 1
        self.width, self.height = self.right - self.left - 1, self.bottom - self.top - 1
        self.confidence = confidence
        self.landmarks = None if landmarks is None else np.asarray(landmarks, np.float32).reshape(5, 2)

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
        self.__detector = _mtcnn.MTCNN(**kwargs).detect_boxes
        self.mode = 'RGB'

    def detector(self, image):
        """The boxes of `detect_faces` (its truncation to integers and its max(0, ...)), each with the float landmarks that
        `detect_faces` truncates."""
        total, points = self.__detector(image)
        boxes = []
        for box, kp in zip(total, points.T):
            x, y = max(0, int(box[0])), max(0, int(box[1]))
            boxes.append(BoundingBox(left=x, top=y, width=int(box[2] - x), height=int(box[3] - y), confidence=box[-1],
                                     landmarks=np.stack([kp[0:5], kp[5:10]], axis=1)))
        return boxes


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
