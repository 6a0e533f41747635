"""Host side of the device face crop, no GPU: the NumPy restatement of Pillow's 8-bit Lanczos resize
(tests/face_crop_oracle.py) against Pillow itself, the window table against image_processing's own numbers, the argument limits,
and the photo_embeddings app with a stubbed detector and network."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
from PIL import Image

from facenet_amd import _lib
from facenet_amd.detectors import face_detector as fd
from facenet_amd.detectors.face_detector import BoundingBox, image_processing
from tests import face_crop_oracle as oracle


def test_oracle_equals_pillow_bit_for_bit():
    cases = list(oracle.random_cases(315, seed=0))
    assert len(cases) >= 300
    kinds = {"up": 0, "down": 0, "non_square": 0, "identity_one": 0, "identity_both": 0, "overhang": 0, "binary": 0}
    mismatches = []
    for i, (frame, window, side) in enumerate(cases):
        left, top, right, bottom = window
        cw, ch, (h, w) = right - left, bottom - top, frame.shape[:2]
        kinds["up"] += cw < side or ch < side
        kinds["down"] += cw > side or ch > side
        kinds["non_square"] += cw != ch
        kinds["identity_one"] += (cw == side) != (ch == side)
        kinds["identity_both"] += cw == side and ch == side
        kinds["overhang"] += left < 0 and top < 0 and right > w and bottom > h
        kinds["binary"] += set(np.unique(frame)) <= {0, 255}
        ref = np.asarray(Image.fromarray(frame).crop(window).resize((side, side), Image.LANCZOS))
        if not np.array_equal(oracle.crop_resize(frame, window, side), ref):
            mismatches.append((i, frame.shape, window, side))
    assert all(v >= 20 for v in kinds.values()), kinds          # every kind of case is in the mix
    assert mismatches == []


def test_oracle_overshoot_is_clipped_on_both_sides():
    """A 0/255 checker of 3-pixel cells drives the Lanczos lobes past both ends of the byte range: the oracle clips like Pillow."""
    cell = np.kron((np.indices((9, 9)).sum(0) % 2).astype(np.uint8) * 255, np.ones((3, 3), np.uint8))
    frame = np.repeat(cell[:, :, None], 3, axis=2)
    taps = oracle.axis_taps(27, 40)[2]
    assert int(taps.min()) < 0 and int(np.clip(taps, 0, None).sum(1).max()) > 1 << oracle.PRECISION_BITS
    ref = np.asarray(Image.fromarray(frame).resize((40, 40), Image.LANCZOS))
    assert np.array_equal(oracle.crop_resize(frame, (0, 0, 27, 27), 40), ref) and ref.min() == 0 and ref.max() == 255


@pytest.mark.parametrize("margin", [0, 0.14, 0.25])
def test_window_table_is_image_processing_arithmetic(margin, monkeypatch):
    opts = SimpleNamespace(size=160, margin=margin)
    boxes = [BoundingBox(30, 20, 50, 60, 0.9), BoundingBox(0, 0, 33, 41), BoundingBox(61.4, 12.6, 21, 25), BoundingBox(-4, 50, 159, 61),
             BoundingBox(3, 4, 10, 18), BoundingBox(7, 9, 50, 54)]       # widths whose margin lands on .5 round half to even
    windows, side, centre = fd.crop_table(boxes, opts)
    assert windows.dtype == np.int32 and windows.shape == (len(boxes), 4)
    assert side == math.ceil(160 + 160 * margin) and centre == (side - 160) // 2
    seen = []

    class Spy(Image.Image):
        def crop(self, window):
            seen.append(tuple(window))
            return self

        def resize(self, size, resample=None):
            seen.append(tuple(size))
            return self
    for box, win in zip(boxes, windows):
        seen.clear()
        image_processing(Spy(), box, opts)
        assert seen == [tuple(int(v) for v in win), (side, side)]
    assert fd.crop_table([], opts)[0].shape == (0, 4)


def test_limits_raise_value_error_before_the_library_is_reached(monkeypatch):
    def no_library():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "load", no_library)
    frame = np.zeros((16, 16, 3), np.uint8)
    ok = np.array([[0, 0, 10, 10]], np.int32)
    e = fd.MAX_EXTENT
    assert fd.MAX_SIDE == 256 and e >= 2048
    fd.check_crop_arguments(ok, 256, 0, 0, 256)
    fd.check_crop_arguments(np.array([[-5, -5, e - 5, e - 5]]), 160, 20, 20, 120)
    for windows, side, ox, oy, s in [
            (ok, 257, 0, 0, 257), (ok, 0, 0, 0, 0), (ok, 16, 0, 0, 0), (ok, 16, 1, 0, 16), (ok, 16, 0, 1, 16), (ok, 16, -1, 0, 8),
            (np.zeros((0, 4), np.int32), 16, 0, 0, 16), (np.array([[0, 0, e + 1, 10]]), 16, 0, 0, 16),
            (np.array([[0, 0, 10, e + 1]]), 16, 0, 0, 16), (np.array([[5, 0, 5, 10]]), 16, 0, 0, 16), (np.array([0, 0, 10, 10]), 16, 0, 0, 16)]:
        with pytest.raises(ValueError):
            fd.crop_resize(frame, windows, side, ox, oy, s)


def test_library_checks_the_same_limits():
    """fn_face_crop_workspace runs on the host: the argument error of the C ABI for the same limits, and the workspace size."""
    import ctypes as C
    lib = _lib.load()
    words = C.c_longlong(0)

    def call(windows, side):
        windows = np.ascontiguousarray(windows, np.int32)
        return lib.fn_face_crop_workspace(windows.ctypes.data, len(windows), side, C.byref(words))
    assert call([[0, 0, 10, 10], [0, 0, 400, 16]], 16) == 0
    kmax = int(math.ceil(3.0 * 400 / 16)) * 2 + 1                  # the widest taps of the batch pad every table
    assert words.value == 4 * 2 + 2 * 2 * 16 * (2 + kmax)
    assert call([[0, 0, fd.MAX_EXTENT, fd.MAX_EXTENT]], 256) == 0 and call([[0, 0, fd.MAX_EXTENT, fd.MAX_EXTENT]], 8) == 0
    for windows, side in [([[0, 0, fd.MAX_EXTENT + 1, 10]], 16), ([[0, 0, 10, fd.MAX_EXTENT + 1]], 16), ([[0, 0, 10, 10]], 257),
                          ([[0, 0, 10, 10]], 0), ([[3, 0, 3, 10]], 16)]:
        assert call(windows, side) == -1
        with pytest.raises(ValueError):
            _lib.check(-1, "face_crop_workspace")


class _StubDetector:
    mode = "RGB"

    def detect(self, frame):
        h, w = frame.shape[:2]
        return [BoundingBox(2, 3, w // 2, h // 2, 0.75), BoundingBox(5, 1, w // 3, h // 3, 0.5)][:1 if h < 50 else 2]


class _StubNet:
    def __init__(self):
        self.batches = []

    def evaluate(self, images):
        self.batches.append(tuple(images.shape))
        flat = np.asarray(images, np.float32).reshape(images.shape[0], -1)
        return np.stack([flat.mean(1), flat.max(1), flat.min(1)], 1)


def _host_crops(frame, boxes, options, centre_crop=False, stream=None):
    import torch
    img = Image.fromarray(np.asarray(frame))
    windows, side, c = fd.crop_table(boxes, options)
    thumbs = [np.asarray(image_processing(img, box, options))[c:c + options.size, c:c + options.size] for box in boxes]
    return torch.from_numpy(np.stack(thumbs)) if thumbs else torch.empty(0, options.size, options.size, 3, dtype=torch.uint8)


def test_photo_embeddings_options_and_npz_layout(tmp_path, monkeypatch):
    from facenet_amd import recognize
    from facenet_amd.apps import photo_embeddings as app
    with pytest.raises(ValueError):
        app.load_options()                                                     # dataset.path is required
    with pytest.raises(ValueError):
        app.load_options(overrides={"dataset": {"path": str(tmp_path)}, "file": "faces.h5"})
    root = tmp_path / "photos"
    rng = np.random.default_rng(0)
    for cls, name, hw in (("alice", "a.png", (64, 80)), ("alice", "b.png", (40, 44)), ("bob", "c.png", (70, 60))):
        (root / cls).mkdir(parents=True, exist_ok=True)
        Image.fromarray(rng.integers(0, 256, hw + (3,), dtype=np.uint8)).save(root / cls / name)
    (root / "bob" / "broken.jpg").write_bytes(b"not an image")
    cfg = tmp_path / "x.yaml"
    cfg.write_text(f"dataset:\n  path: {root}\nimage:\n  size: 32\n  margin: 0.25\nmtcnn:\n  weights_file: w.npz\n")
    opts = app.load_options(cfg)
    assert opts.image.size == 32 and opts.image.margin == 0.25 and opts.detector == "pypimtcnn" and opts.mtcnn.weights_file == "w.npz"
    assert opts.model.normalize is True and opts.file == tmp_path / "photos_model" / "photo_embeddings.npz"
    opts = app.load_options(cfg, overrides={"file": str(tmp_path / "out" / "faces.npz")})

    monkeypatch.setattr(recognize, "image_processing_batch", _host_crops)
    net = _StubNet()
    pipeline = recognize.FacePipeline(_StubDetector(), net, opts.image, device="cpu")
    out = app.write_photo_embeddings(opts, pipeline=pipeline, log=lambda *a: None)
    z = np.load(out)
    assert sorted(z.files) == ["boxes", "confidence", "embeddings", "face", "files"]
    names = [str(root / "alice" / "a.png")] * 2 + [str(root / "alice" / "b.png")] + [str(root / "bob" / "c.png")] * 2
    assert [str(f) for f in z["files"]] == names and z["face"].tolist() == [0, 1, 0, 0, 1]
    assert z["boxes"].shape == (5, 4) and z["boxes"][0].tolist() == [2, 3, 40, 32] and z["boxes"][2].tolist() == [2, 3, 22, 20]
    assert z["confidence"].tolist() == [0.75, 0.5, 0.75, 0.75, 0.5]
    assert z["embeddings"].shape == (5, 3) and z["embeddings"].dtype == np.float32
    assert net.batches == [(4, 32, 32, 3), (1, 32, 32, 3), (4, 32, 32, 3)]      # 2 faces share the plan of 4, 1 face has its own
    frame = np.asarray(Image.open(root / "alice" / "b.png"))
    crop = _host_crops(frame, _StubDetector().detect(frame), opts.image).numpy().astype(np.float32)
    assert z["embeddings"][2].tolist() == [crop.mean(dtype=np.float32), crop.max(), crop.min()]


def test_extract_faces_keeps_its_default(tmp_path):
    """device_resize is off unless asked for: the PIL route runs, nothing touches a device."""
    import inspect

    from facenet_amd.apps.extract_faces import extract_faces
    assert inspect.signature(extract_faces).parameters["device_resize"].default is False
    src = tmp_path / "in" / "alice"
    src.mkdir(parents=True)
    Image.fromarray(np.random.default_rng(1).integers(0, 256, (64, 80, 3), dtype=np.uint8)).save(src / "a.png")
    cls = SimpleNamespace(name="alice", files=[str(src / "a.png")])
    opts = SimpleNamespace(size=32, margin=0.25)
    stats = extract_faces([cls], tmp_path / "out", _StubDetector(), opts, detect_multiple_faces=True, log=lambda *a: None)
    assert stats["extracted"] == 1 and sorted(p.name for p in (tmp_path / "out" / "alice").iterdir()) == ["a.png", "a_1.png"]
    box = _StubDetector().detect(np.zeros((64, 80, 3)))[1]
    ref = np.asarray(image_processing(Image.open(src / "a.png"), box, opts))
    assert np.array_equal(np.asarray(Image.open(tmp_path / "out" / "alice" / "a_1.png")), ref)
