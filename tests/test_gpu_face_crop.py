"""fn_face_crop_resize_u8 and what is built on it on the GPU.  The reference is Pillow itself:
`Image.fromarray(frame).crop(window).resize((side, side), Image.LANCZOS)`, and every comparison is bit equality."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch
from PIL import Image

from facenet_amd import _lib
from facenet_amd.detectors import face_detector as fd
from facenet_amd.detectors import mtcnn as gm
from facenet_amd.detectors.face_detector import BoundingBox, FaceDetector, image_processing, image_processing_batch
from oracle import mtcnn_oracle as mo

pytestmark = pytest.mark.gpu
FACE_BIAS = (0.5, 1.0, 1.0)     # the synthetic detector of tests/test_gpu_mtcnn.py: every stage passes some candidates


def _frame(h, w, seed=0, cell=8):
    """Blocky random image + noise (the frame of tests/test_gpu_mtcnn.py)."""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (-(-h // cell), -(-w // cell), 3), dtype=np.uint8)
    img = np.kron(base, np.ones((cell, cell, 1), np.uint8))[:h, :w].astype(np.int32) + rng.integers(-12, 13, (h, w, 3))
    return np.clip(img, 0, 255).astype(np.uint8)


def _pillow(frame, window, side):
    return np.asarray(Image.fromarray(frame).crop(tuple(int(v) for v in window)).resize((side, side), Image.LANCZOS))


def _windows(h, w, side):
    """One launch's windows: tap counts from 1 (copy) to the whole frame squeezed into `side`, so the padded tables are exercised."""
    big = round(2.5 * side)
    return np.array([
        (w // 2 - big // 2, h // 2 - big // 2, w // 2 - big // 2 + big, h // 2 - big // 2 + big),    # ~2.5x downscale about the centre
        (-3, -2, w + 4, h + 5),                        # overhangs all four sides
        (11, 7, 31, 27),                               # a 20-pixel box (an upscale at sides 160 and 200)
        (5, 3, 5 + side, 3 + 37),                      # crop width == side: the horizontal pass is skipped
        (2, 1, 2 + 29, 1 + side),                      # crop height == side: the vertical pass is skipped
        (-5, 3, -5 + side, 3 + side),                  # both extents == side: pure copy
        (-7, -9, 30, 25),                              # negative left / top only
        (w - 25, h - 20, w + 9, h + 11),               # right / bottom overhang only
        (w + 3, h + 2, w + 40, h + 30),                # fully outside the frame: all zeros
        (10, 5, 11, 35),                               # 1 pixel wide
        (2, 3, 2 + 90, 3 + 14),                        # strongly non-square
    ], np.int32)


@pytest.mark.parametrize("side", [8, 160, 200])
@pytest.mark.parametrize("binary", [False, True], ids=["bytes", "0-255"])
@pytest.mark.parametrize("hw", [(40, 56), (97, 131), (120, 160)])
def test_kernel_equals_pillow(hw, binary, side):
    rng = np.random.default_rng(hw[0] * 1000 + side + binary)
    frame = (rng.integers(0, 2, hw + (3,)) * 255).astype(np.uint8) if binary else rng.integers(0, 256, hw + (3,), dtype=np.uint8)
    windows = _windows(hw[0], hw[1], side)
    got = fd.crop_resize(frame, windows, side).cpu()
    assert got.shape == (len(windows), side, side, 3) and got.dtype == torch.uint8
    for i, win in enumerate(windows):
        ref = torch.from_numpy(_pillow(frame, win, side).copy())
        assert torch.equal(got[i], ref), (i, win.tolist(), int((got[i].int() - ref.int()).abs().max()), int((got[i] != ref).sum()))
    assert int(got[8].max()) == 0                      # the window outside the frame


def test_output_window_is_the_slice_of_the_full_result():
    frame = _frame(120, 160, seed=3)
    windows = _windows(120, 160, 200)
    full = fd.crop_resize(torch.from_numpy(frame).cuda(), windows, 200)
    part = fd.crop_resize(torch.from_numpy(frame).cuda(), windows, 200, 20, 20, 160)
    assert part.shape == (len(windows), 160, 160, 3)
    assert torch.equal(part, full[:, 20:180, 20:180])
    odd = fd.crop_resize(frame, windows, 200, 3, 31, 57)       # an offset and a size that are no multiple of anything
    assert torch.equal(odd, full[:, 31:88, 3:60])


@pytest.mark.parametrize("side", [8, 256])
def test_window_at_the_documented_maximum_extent(side, monkeypatch):
    """MAX_EXTENT pixels per axis is the most one output row's taps may span (the LDS plan of section 17): sides 8 and 256 are
    the two ends of that plan (most rows per output row; widest rows)."""
    frame = _frame(64, 64, seed=5)
    e = fd.MAX_EXTENT
    win = np.array([[-1000, -1500, -1000 + e, -1500 + e]], np.int32)
    got = fd.crop_resize(frame, win, side).cpu()
    assert torch.equal(got[0], torch.from_numpy(_pillow(frame, win[0], side).copy()))

    def no_library():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "load", no_library)              # ValueError before anything could be launched
    for beyond in ([[-1000, -1500, -1000 + e + 1, -1500 + e]], [[-1000, -1500, -1000 + e, -1500 + e + 1]]):
        with pytest.raises(ValueError):
            fd.crop_resize(frame, np.array(beyond, np.int32), side)


def test_entry_point_rejects_bad_arguments(lib):
    """C-ABI error behaviour: rc = FN_EINVAL (-> ValueError) with a message, nothing launched."""
    import ctypes as C
    frame = torch.zeros(16, 16, 3, dtype=torch.uint8, device="cuda")
    dst = torch.zeros(256 * 256 * 3, dtype=torch.uint8, device="cuda")
    work = torch.zeros(1 << 16, dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def call(win, F, side, ox, oy, S, words=work.numel()):
        win = np.asarray(win, np.int32)
        return lib.fn_face_crop_resize_u8(frame.data_ptr(), 16, 16, win.ctypes.data, F, side, ox, oy, S, dst.data_ptr(), work.data_ptr(), words, st)
    ok = [[0, 0, 10, 10]]
    assert call(ok, 1, 16, 0, 0, 16) == 0
    for bad in [(ok, 0, 16, 0, 0, 16), (ok, 1, 257, 0, 0, 16), (ok, 1, 16, 0, 0, 0), (ok, 1, 16, 1, 0, 16), (ok, 1, 16, 0, 1, 16),
                (ok, 1, 16, -1, 0, 8), ([[0, 0, fd.MAX_EXTENT + 1, 10]], 1, 16, 0, 0, 16), ([[0, 0, 0, 10]], 1, 16, 0, 0, 16),
                (ok, 1, 16, 0, 0, 16, 8)]:
        assert call(*bad) == -1 and lib.fn_last_error()
    words = C.c_longlong(0)
    win = np.asarray(ok, np.int32)
    assert lib.fn_face_crop_workspace(win.ctypes.data, 1, 16, C.byref(words)) == 0 and words.value == 4 + 2 * 16 * (2 + 7)
    torch.cuda.synchronize()


def _boxes(h, w):
    return [BoundingBox(30, 20, 50, 60, 0.9), BoundingBox(0, 0, 33, 41, 0.8), BoundingBox(w - 40, h - 35, 39, 34, 0.7),
            BoundingBox(61.4, 12.6, 20, 24, 0.6), BoundingBox(-4, 50, 159, 60, 0.5)]


@pytest.mark.parametrize("margin", [0, 0.25])
def test_batch_wrapper_equals_image_processing(margin):
    frame = _frame(120, 160, seed=2)
    img = Image.fromarray(frame)
    opts = SimpleNamespace(size=160, margin=margin)
    boxes = _boxes(120, 160)
    got = image_processing_batch(frame, boxes, opts).cpu().numpy()
    cut = image_processing_batch(torch.from_numpy(frame).cuda(), boxes, opts, centre_crop=True).cpu().numpy()
    side = 160 if margin == 0 else 200
    assert got.shape == (len(boxes), side, side, 3) and cut.shape == (len(boxes), 160, 160, 3)
    c = (side - 160) // 2
    for i, box in enumerate(boxes):
        ref = np.asarray(image_processing(img, box, opts))
        assert np.array_equal(got[i], ref), i
        assert np.array_equal(cut[i], ref[c:c + 160, c:c + 160]), i
    assert image_processing_batch(frame, [], opts, centre_crop=True).shape == (0, 160, 160, 3)


@pytest.fixture(scope="module")
def weights():
    return mo.random_weights(0, face_bias=FACE_BIAS)


@pytest.fixture(scope="module")
def detector(weights, tmp_path_factory):
    path = tmp_path_factory.mktemp("mtcnn") / "w.npz"
    np.savez(path, **weights)
    return FaceDetector(detector="pypimtcnn", weights_file=str(path)), str(path)


def test_extract_faces_device_resize_writes_the_same_thumbnails(detector, tmp_path):
    from facenet_amd.apps.extract_faces import extract_faces
    src = tmp_path / "in" / "alice"
    src.mkdir(parents=True)
    Image.fromarray(_frame(120, 160, seed=1)).save(src / "a.png")
    Image.fromarray(np.zeros((11, 30, 3), np.uint8)).save(src / "tiny.png")
    (src / "broken.jpg").write_bytes(b"not an image")
    cls = SimpleNamespace(name="alice", files=sorted(str(p) for p in src.iterdir()))
    opts = SimpleNamespace(size=160, margin=0.25)
    runs = {}
    for device_resize in (False, True):
        out = tmp_path / f"out{int(device_resize)}"
        stats = extract_faces([cls], out, detector[0], opts, detect_multiple_faces=True, log=lambda *a: None, device_resize=device_resize)
        files = sorted(p.name for p in (out / "alice").iterdir())
        runs[device_resize] = (stats, files, [np.asarray(Image.open(out / "alice" / f)) for f in files])
    assert runs[True][0] == runs[False][0] and runs[True][1] == runs[False][1] and len(runs[True][1]) > 1
    for name, a, b in zip(runs[True][1], runs[True][2], runs[False][2]):
        assert a.shape == (200, 200, 3) and np.array_equal(a, b), name


@pytest.fixture(scope="module")
def pipeline(detector):
    from facenet_amd.api import FaceNet
    from facenet_amd.config import Config
    from facenet_amd.recognize import FacePipeline
    facenet = FaceNet(Config({"normalize": True, "embedding_size": 128, "image": {"size": 160, "normalization": 0}}))
    return FacePipeline(detector[0], facenet, SimpleNamespace(size=160, margin=0.25))


def test_face_pipeline(pipeline, monkeypatch):
    from facenet_amd.recognize import padded_batch
    frame = _frame(120, 160, seed=1)
    img = Image.fromarray(frame)
    boxes, crops = pipeline.crops(frame)
    expect = pipeline.detector.detect(frame)
    assert len(boxes) == len(expect) > 1 and [b.info() for b in boxes] == [b.info() for b in expect]
    assert crops.is_cuda and crops.dtype == torch.uint8 and crops.shape == (len(boxes), 160, 160, 3)
    ref = np.stack([np.asarray(image_processing(img, box, pipeline.image_options))[20:180, 20:180] for box in boxes])
    assert np.array_equal(crops.cpu().numpy(), ref)                    # the Pillow route followed by the centre cut

    faces = pipeline.faces(frame)
    assert [b.info() for b, _ in faces] == [b.info() for b in boxes]
    n = padded_batch(len(boxes))
    assert [padded_batch(k) for k in (1, 2, 3, 4, 5, 16, 17, 256, 257)] == [1, 4, 4, 4, 16, 16, 64, 256, 512] and n >= len(boxes)
    batch = np.zeros((n, 160, 160, 3), np.uint8)
    batch[:len(boxes)] = ref
    want = pipeline.facenet.evaluate(batch)[:len(boxes)]
    got = np.stack([e for _, e in faces])
    assert got.dtype == np.float32 and got.shape == (len(boxes), 128)
    assert np.array_equal(got, want)                                    # the same uint8 batch at the same padded batch size

    def no_network(images):
        raise AssertionError("the network ran without a face")
    monkeypatch.setattr(pipeline.facenet, "evaluate", no_network)
    assert pipeline.faces(np.zeros((11, 30, 3), np.uint8)) == []       # smaller than one 12x12 cell at every scale


def test_photo_embeddings_app(detector, tmp_path):
    """`python -m facenet_amd.apps.photo_embeddings --config x.yaml` on a two-image data set (entered through its click command)."""
    import yaml
    from click.testing import CliRunner

    from facenet_amd.apps import photo_embeddings as app
    src = tmp_path / "photos" / "alice"
    src.mkdir(parents=True)
    Image.fromarray(_frame(120, 160, seed=1)).save(src / "a.png")
    Image.fromarray(_frame(97, 131, seed=4)).save(src / "b.png")
    cfg = tmp_path / "x.yaml"
    out = tmp_path / "result" / "faces.npz"
    cfg.write_text(yaml.safe_dump({"dataset": {"path": str(tmp_path / "photos")}, "model": {"normalize": True, "embedding_size": 128},
                                   "image": {"size": 160, "margin": 0.25}, "mtcnn": {"weights_file": detector[1]}, "file": str(out)}))
    result = CliRunner().invoke(app.main, ["--config", str(cfg)], catch_exceptions=False)
    assert result.exit_code == 0, result.output
    z = np.load(out)
    n = len(z["files"])
    per_photo = {name: len(detector[0].detect(np.asarray(Image.open(src / name)))) for name in ("a.png", "b.png")}
    assert n == sum(per_photo.values()) > 1
    assert z["embeddings"].shape == (n, 128) and z["embeddings"].dtype == np.float32 and z["boxes"].shape == (n, 4)
    assert z["confidence"].shape == (n,) and z["face"].shape == (n,)
    assert [str(f) for f in z["files"]] == [str(src / name) for name in ("a.png", "b.png") for _ in range(per_photo[name])]
    assert z["face"].tolist() == [i for name in ("a.png", "b.png") for i in range(per_photo[name])]
    assert np.allclose(np.linalg.norm(z["embeddings"], axis=1), 1.0, atol=1e-3)
