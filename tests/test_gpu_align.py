"""fn_face_align_u8 and what is built on it on the GPU.  The reference is tests/align_oracle.py, and every
pixel comparison is bit equality with its bytes.  The detector's weights in this repository are synthetic, so its landmarks are no
faces: the kernel tests plant their transforms, and the pipeline tests check that whatever the detector returned is carried
through and used exactly."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch
from PIL import Image

from facenet_amd.detectors import face_detector as fd
from facenet_amd.detectors.face_detector import BoundingBox, FaceDetector, image_processing_aligned_batch, image_processing_batch
from oracle import mtcnn_oracle as mo
from tests import align_oracle as ao

pytestmark = pytest.mark.gpu
FACE_BIAS = (0.5, 1.0, 1.0)     # the synthetic detector of tests/test_gpu_face_crop.py: every stage passes some candidates
GUARD = 64                      # bytes behind dst that no launch may touch


def _frame(h, w, seed=0, cell=8):
    """Blocky random image + noise (the frame of tests/test_gpu_face_crop.py)."""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (-(-h // cell), -(-w // cell), 3), dtype=np.uint8)
    img = np.kron(base, np.ones((cell, cell, 1), np.uint8))[:h, :w].astype(np.int32) + rng.integers(-12, 13, (h, w, 3))
    return np.clip(img, 0, 255).astype(np.uint8)


def _faces(h, w, S):
    """One launch's faces: (what, the six inverse entries, n)."""
    mid = ((w - 1) / 2, (h - 1) / 2)
    over = 0.5 * min(h, w) / S                                   # a footprint of half the frame, centred on each border in turn
    faces = [
        ("copy", [1, 0, 3, 0, 1, 2], 1),
        ("30 degrees, sigma 1.7", ao.inverse_of(1.7, math.radians(30), mid, S), 2),
        ("sigma 0.4: an upscale", ao.inverse_of(0.4, -0.7, mid, S), 1),
        ("sigma 7.9", ao.inverse_of(7.9, 0.1, mid, S), 8),
        ("sigma 8.5: n capped at 8", ao.inverse_of(8.5, -0.2, mid, S), 8),
        ("180 degrees", ao.inverse_of(1.0, math.pi, mid, S), 1),
        ("over the left border", ao.inverse_of(over, 0.2, (0, mid[1]), S), ao.samples_of(over)),
        ("over the right border", ao.inverse_of(over, 0.2, (w - 1, mid[1]), S), ao.samples_of(over)),
        ("over the top border", ao.inverse_of(over, 0.2, (mid[0], 0), S), ao.samples_of(over)),
        ("over the bottom border", ao.inverse_of(over, 0.2, (mid[0], h - 1), S), ao.samples_of(over)),
        ("outside the frame", ao.inverse_of(1.0, 0.3, (-300, -300), S), 1),
        ("integer source coordinates, n = 2", [4, 0, 3, 0, 4, 1], 2),     # sub-samples at u -+ 0.25: x = 4 u -+ 1 + 3
        ("integer source coordinates, a quarter turn", [0, -1, w - 2, 1, 0, 1], 1),
        ("3 samples per axis", ao.inverse_of(2.6, 2.0, mid, S), 3),
    ]
    assert ao.samples_of(1.7) == 2 and ao.samples_of(0.4) == 1 and ao.samples_of(7.9) == 8 and ao.samples_of(8.5) == 8
    return faces


def _launch(lib, frame, inverse, samples, S, guard=GUARD):
    """The C entry on a dst with guard bytes behind it -> (rc, uint8 [F, S, S, 3] on the host, the guard bytes)."""
    import ctypes as C
    inverse, samples = np.ascontiguousarray(inverse, np.float64), np.ascontiguousarray(samples, np.int32)
    F = len(samples)
    nbytes = C.c_longlong(0)
    assert lib.fn_face_align_workspace(F, C.byref(nbytes)) == 0 and nbytes.value >= F * 52 and nbytes.value % 8 == 0
    work = torch.empty(nbytes.value // 8, dtype=torch.int64, device="cuda")
    dev = torch.from_numpy(frame).cuda()
    dst = torch.full((F * S * S * 3 + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    rc = lib.fn_face_align_u8(dev.data_ptr(), frame.shape[0], frame.shape[1], inverse.ctypes.data, samples.ctypes.data, F, S, dst.data_ptr(),
                              work.data_ptr(), nbytes.value, torch.cuda.current_stream().cuda_stream)
    out = dst.cpu().numpy()
    return rc, out[:F * S * S * 3].reshape(F, S, S, 3), out[F * S * S * 3:]


@pytest.mark.parametrize("S", [8, 113, 160])
@pytest.mark.parametrize("hw", [(40, 56), (97, 131)])
def test_kernel_equals_the_oracle(lib, hw, S):
    frame = np.random.default_rng(hw[0] + S).integers(0, 256, hw + (3,), dtype=np.uint8)
    faces = _faces(hw[0], hw[1], S)
    rc, got, guard = _launch(lib, frame, [f[1] for f in faces], [f[2] for f in faces], S)
    assert rc == 0, lib.fn_last_error()
    assert (guard == 0xA5).all()
    for i, (what, inverse, n) in enumerate(faces):
        ref = ao.warp(frame, inverse, n, S)
        assert np.array_equal(got[i], ref), (what, int(np.abs(got[i].astype(int) - ref).max()), int((got[i] != ref).sum()))
    assert np.array_equal(got[0][:min(S, hw[0] - 2), :min(S, hw[1] - 3)], frame[2:2 + S, 3:3 + S])      # the copy is a slice of the frame
    assert got[10].max() == 0                                                                        # outside: all zeros
    assert got[6].max() > 0 and got[1].max() > 0


def test_one_face_through_align_faces(lib):
    frame = _frame(97, 131, seed=6)
    inverse = ao.inverse_of(1.7, math.radians(30), (70.0, 50.0), 160)
    one = fd.Alignment(np.array([inverse]), np.array([2], np.int32), np.array([True]), np.zeros(1), np.ones(1), np.zeros(1))
    got = fd.align_faces(frame, one, 160)
    assert got.is_cuda and got.dtype == torch.uint8 and got.shape == (1, 160, 160, 3)
    assert np.array_equal(got[0].cpu().numpy(), ao.warp(frame, inverse, 2, 160))
    rc, direct, guard = _launch(lib, frame, [inverse], [2], 160)
    assert rc == 0 and (guard == 0xA5).all() and np.array_equal(direct, got.cpu().numpy())


def test_entry_point_rejects_bad_arguments(lib):
    """C-ABI error behaviour: rc = FN_EINVAL with a message, nothing launched (dst keeps its fill)."""
    import ctypes as C
    frame = torch.zeros(16, 16, 3, dtype=torch.uint8, device="cuda")
    dst = torch.full((2 * 16 * 16 * 3,), 0xA5, dtype=torch.uint8, device="cuda")
    work = torch.zeros(1 << 17, dtype=torch.int64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    good = [1.0, 0, 0, 0, 1, 0]
    keep = []

    def call(inverse=(good, good), samples=(1, 2), F=2, S=16, H=16, W=16, nbytes=work.numel() * 8, frame_p=frame.data_ptr(), dst_p=dst.data_ptr(),
             work_p=work.data_ptr(), null=()):
        inverse, samples = np.ascontiguousarray(inverse, np.float64), np.ascontiguousarray(samples, np.int32)
        keep[:] = [inverse, samples]
        return lib.fn_face_align_u8(frame_p, H, W, None if "inverse" in null else inverse.ctypes.data, None if "samples" in null else samples.ctypes.data,
                                    F, S, dst_p, work_p, nbytes, st)
    many = dict(inverse=np.tile(good, (65536, 1)), samples=np.ones(65536, np.int32), F=65536)
    bad = [dict(frame_p=None), dict(dst_p=None), dict(work_p=None), dict(null=("inverse",)), dict(null=("samples",)), dict(H=0), dict(W=0),
           dict(F=0), many, dict(S=0), dict(S=257), dict(samples=(1, 0)), dict(samples=(9, 1)), dict(nbytes=2 * 52 - 1),
           dict(work_p=work.data_ptr() + 4)]
    for entry in (math.nan, math.inf, -math.inf, 2.0 ** 24, -(2.0 ** 24)):
        for k in (0, 2, 5):
            row = list(good)
            row[k] = entry
            bad.append(dict(inverse=(good, row)))
    for kw in bad:
        assert call(**kw) == -1 and lib.fn_last_error(), kw
    torch.cuda.synchronize()
    assert bool((dst == 0xA5).all())
    assert call(inverse=(good, [1, 0, 2.0 ** 24 - 1, 0, 1, 0])) == 0          # the largest entry that passes
    torch.cuda.synchronize()
    assert not bool((dst == 0xA5).all())
    nbytes = C.c_longlong(0)
    assert lib.fn_face_align_workspace(0, C.byref(nbytes)) == -1 and lib.fn_face_align_workspace(65536, C.byref(nbytes)) == -1
    assert lib.fn_face_align_workspace(3, None) == -1
    assert lib.fn_face_align_workspace(3, C.byref(nbytes)) == 0 and nbytes.value == 160


def test_side_at_its_maximum(lib):
    frame = _frame(40, 56, seed=7)
    inverse = ao.inverse_of(0.2, 0.5, (28.0, 20.0), 256)
    rc, got, guard = _launch(lib, frame, [inverse], [1], 256)
    assert rc == 0 and (guard == 0xA5).all() and np.array_equal(got[0], ao.warp(frame, inverse, 1, 256))


OPTIONS = SimpleNamespace(size=160, margin=0.25)


def _expected(frame, boxes, options=OPTIONS):
    """What `image_processing_aligned_batch` must return: the oracle's fit and warp for every box whose own landmarks are
    alignable, the box path's bytes for the others -> (uint8 [F, size, size, 3], ok flags)."""
    template = ao.align_template(options.size, options.margin)
    rows, flags = [], []
    for box in boxes:
        fit = ao.fit(box.landmarks, template, options.size) if box.landmarks is not None else {"ok": False}
        flags.append(fit["ok"])
        if fit["ok"]:
            rows.append(ao.warp(frame, fit["inverse"], fit["samples"], options.size))
        else:
            rows.append(image_processing_batch(frame, [box], options, centre_crop=True)[0].cpu().numpy())
    return np.stack(rows), flags


def test_batch_wrapper_with_planted_landmarks():
    frame = _frame(120, 160, seed=2)
    template = ao.align_template(160, 0.25)
    planted = ao.landmarks_of(ao.inverse_of(0.45, math.radians(-20), (62.0, 55.0), 160), template)
    planted += np.random.default_rng(8).normal(0, 0.15, (5, 2))                   # no exact similarity: a residual to report
    boxes = [BoundingBox(30, 20, 50, 60, 0.9, landmarks=planted), BoundingBox(0, 0, 33, 41, 0.8),
             BoundingBox(100, 60, 39, 34, 0.7, landmarks=np.full((5, 2), 120.0))]
    got, alignment = image_processing_aligned_batch(torch.from_numpy(frame).cuda(), boxes, OPTIONS)
    assert got.is_cuda and got.dtype == torch.uint8 and got.shape == (3, 160, 160, 3)
    assert alignment.ok.tolist() == [True, False, False] and alignment.samples.tolist() == [1, 0, 0]
    assert 0 < alignment.residual[0] < 0.01 and abs(alignment.angle[0] - 20) < 2 and abs(alignment.scale[0] - 1 / 0.45) < 0.05
    want, flags = _expected(frame, boxes)
    assert flags == [True, False, False]
    assert np.array_equal(got.cpu().numpy(), want)
    assert not np.array_equal(want[0], image_processing_batch(frame, boxes[:1], OPTIONS, centre_crop=True)[0].cpu().numpy())
    every, _ = image_processing_aligned_batch(frame, boxes[:1] * 2, OPTIONS)         # all rows aligned, the frame as an array
    assert np.array_equal(every.cpu().numpy(), want[[0, 0]])
    none, _ = image_processing_aligned_batch(frame, boxes[1:], OPTIONS)              # no row aligned
    assert np.array_equal(none.cpu().numpy(), want[1:])
    empty, nobody = image_processing_aligned_batch(frame, [], OPTIONS)
    assert empty.shape == (0, 160, 160, 3) and len(nobody) == 0


@pytest.fixture(scope="module")
def detector(tmp_path_factory):
    path = tmp_path_factory.mktemp("mtcnn") / "w.npz"
    np.savez(path, **mo.random_weights(0, face_bias=FACE_BIAS))
    return FaceDetector(detector="pypimtcnn", weights_file=str(path)), str(path)


@pytest.fixture(scope="module")
def photo(detector):
    """One photograph, its detected boxes and the bytes every aligned route must produce for them."""
    frame = _frame(120, 160, seed=1)
    boxes = detector[0].detect(frame)
    want, flags = _expected(frame, boxes)
    return frame, boxes, want, flags


def test_detector_carries_the_float_landmarks(detector, photo):
    from facenet_amd.detectors import mtcnn as gm
    frame, boxes, _, _ = photo
    total, points = gm.MTCNN(weights_file=detector[1]).detect_boxes(frame)
    assert len(boxes) == len(total) > 1 and points.dtype == np.float32
    for box, row, kp in zip(boxes, total, points.T):
        assert box.landmarks.dtype == np.float32 and np.array_equal(box.landmarks, np.stack([kp[:5], kp[5:]], axis=1))
        x, y = max(0, int(row[0])), max(0, int(row[1]))                            # the boxes detect_faces builds
        assert box.info() == BoundingBox(x, y, int(row[2] - x), int(row[3] - y), row[-1]).info()


def test_face_pipeline_aligned_crops(detector, photo):
    from facenet_amd.recognize import FacePipeline
    frame, _, want, flags = photo
    plain_boxes, plain = FacePipeline(detector[0], None, OPTIONS).crops(frame)
    boxes, crops = FacePipeline(detector[0], None, OPTIONS, align=True).crops(frame)
    assert [b.info() for b in boxes] == [b.info() for b in plain_boxes] and len(boxes) == len(want) > 1
    assert crops.is_cuda and crops.dtype == torch.uint8 and np.array_equal(crops.cpu().numpy(), want)
    print("alignable faces", sum(flags), "of", len(flags))
    for i, ok in enumerate(flags):                                                 # the rows that fell back are the box path's rows
        assert ok or torch.equal(crops[i], plain[i])
    _, _, alignment = FacePipeline(detector[0], None, SimpleNamespace(size=160, margin=0.25, align=True)).aligned_crops(frame)
    assert alignment.ok.tolist() == flags


def test_extract_faces_writes_the_aligned_thumbnails(detector, photo, tmp_path):
    from facenet_amd.apps.extract_faces import extract_faces
    frame, boxes, want, _ = photo
    src = tmp_path / "in" / "alice"
    src.mkdir(parents=True)
    Image.fromarray(frame).save(src / "a.png")
    cls = SimpleNamespace(name="alice", files=[str(src / "a.png")])
    stats = extract_faces([cls], tmp_path / "out", detector[0], OPTIONS, detect_multiple_faces=True, log=lambda *a: None, align=True)
    assert stats["extracted"] == 1 and len(stats["sizes"]) == len(boxes)
    for n in range(len(boxes)):
        thumb = np.asarray(Image.open(tmp_path / "out" / "alice" / ("a.png" if n == 0 else f"a_{n}.png")))
        assert thumb.shape == (160, 160, 3) and np.array_equal(thumb, want[n]), n
