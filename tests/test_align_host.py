"""Landmark alignment on the host: the definition in tests/align_oracle.py against independent
implementations (numpy.linalg.lstsq for the fit, Pillow's affine transform for the warp's geometry), the host arithmetic of
facenet_amd.detectors.face_detector against that definition, and the argument rules that hold before the library is reached."""
import math
from fractions import Fraction
from types import SimpleNamespace

import numpy as np
import pytest
import torch
from PIL import Image

from facenet_amd import _lib, recognize
from facenet_amd.config import Config
from facenet_amd.detectors import face_detector as fd
from tests import align_oracle as ao


def _random_landmarks(rng, count, size=112, near_origin=False):
    """Templates moved by a random similarity plus landmark noise, every coordinate within +-1e3: faces of 20 .. 700 pixels
    somewhere in a 1000 x 1000 frame, or with near_origin centred within 100 pixels of (0, 0)."""
    template = ao.align_template(size)
    out = np.empty((count, 5, 2))
    for k in range(count):
        sigma, angle = math.exp(rng.uniform(math.log(0.2), math.log(6.0))), rng.uniform(-math.pi, math.pi)
        half = sigma * size * 0.75
        centre = rng.uniform(half, 1000 - half, 2) if half < 500 else np.array([500.0, 500.0])
        if near_origin:
            centre = rng.uniform(-100, 100, 2)
        out[k] = ao.landmarks_of(ao.inverse_of(sigma, angle, centre, size), template) + rng.normal(0, 0.02 * sigma * size, (5, 2))
    return np.clip(out, -1000, 1000)


def _lstsq(p, q):
    """(a, b, tx, ty) of the 10 x 4 linear system M p_i + t = q_i."""
    A = np.zeros((10, 4))
    A[0::2, 0], A[0::2, 1], A[0::2, 2] = p[:, 0], -p[:, 1], 1
    A[1::2, 0], A[1::2, 1], A[1::2, 3] = p[:, 1], p[:, 0], 1
    return np.linalg.lstsq(A, q.reshape(-1), rcond=None)[0]


def _exact(p, q):
    """(a, b, tx, ty) of the closed form in rational arithmetic on the same doubles, rounded once at the end."""
    p, q = ([[Fraction(float(c)) for c in row] for row in pts] for pts in (p, q))
    pmx, pmy, qmx, qmy = (sum(row[i] for row in pts) / 5 for pts in (p, q) for i in (0, 1))
    den = sum((x - pmx) ** 2 + (y - pmy) ** 2 for x, y in p)
    a = sum((px - pmx) * (qx - qmx) + (py - pmy) * (qy - qmy) for (px, py), (qx, qy) in zip(p, q)) / den
    b = sum((px - pmx) * (qy - qmy) - (py - pmy) * (qx - qmx) for (px, py), (qx, qy) in zip(p, q)) / den
    return np.array([float(a), float(b), float(qmx - (a * pmx - b * pmy)), float(qmy - (b * pmx + a * pmy))])


def test_fit_equals_least_squares():
    """The closed form against numpy.linalg.lstsq on the 10 x 4 system, absolute 1e-9, 200 random cases with inputs of magnitude
    <= 1e3.  lstsq solves the UNcentred system, whose condition number grows as the face's distance from the origin over its
    size: for a 28-pixel face 800 pixels out lstsq itself is 6e-8 away from the exact solution (the closed form: 1e-12), so this
    comparison draws its faces around the origin, where lstsq is good to the bound ..."""
    rng = np.random.default_rng(0)
    template = ao.align_template(112)
    worst = 0.0
    for p in _random_landmarks(rng, 200, near_origin=True):
        assert np.abs(p).max() <= 1e3
        got = ao.fit(p, template)
        assert got["ok"]
        worst = max(worst, float(np.abs(np.asarray(got["forward"]) - _lstsq(p, template)).max()))
    print("worst |closed form - lstsq|", worst)
    assert worst <= 1e-9


def test_fit_equals_exact_arithmetic_anywhere_in_the_frame():
    """... and faces anywhere in a 1000 x 1000 frame are held to the closed form in rational arithmetic.  The entries reach 7e3
    (a translation of scale 5 times 1e3 sqrt 2), where one rounding is 4.5e-13; the fit takes about a dozen in sequence: 1e-11."""
    rng = np.random.default_rng(4)
    template = ao.align_template(112)
    worst = 0.0
    for p in _random_landmarks(rng, 200):
        worst = max(worst, float(np.abs(np.asarray(ao.fit(p, template)["forward"]) - _exact(p, template)).max()))
    print("worst |closed form - exact|", worst)
    assert worst <= 1e-11


def test_host_fit_is_the_definition():
    """similarity_from_landmarks is the oracle's arithmetic in the oracle's order: the same doubles, not nearly the same."""
    rng = np.random.default_rng(1)
    for size, margin in ((112, 0), (160, 0.25)):
        template = fd.align_template(size, margin)
        assert np.array_equal(template, ao.align_template(size, margin))
        points = _random_landmarks(rng, 200, size).astype(np.float32)           # what BoundingBox.landmarks holds
        points[7, 3, 1] = np.nan
        points[11] = points[11, 0]
        got = fd.similarity_from_landmarks(points, template, size)
        assert len(got) == 200 and got.inverse.shape == (200, 6) and got.inverse.dtype == np.float64 and got.samples.dtype == np.int32
        for k, p in enumerate(points):
            ref = ao.fit(p, template, size)
            assert bool(got.ok[k]) == ref["ok"] and got.samples[k] == ref["samples"], k
            assert np.array_equal(got.inverse[k], ref["inverse"], equal_nan=True), k
            if ref["ok"]:
                assert got.residual[k] == ref["residual"] and got.scale[k] == ref["scale"] and abs(got.angle[k] - ref["angle"]) < 1e-11, k
        assert not got.ok[7] and not got.ok[11] and got.ok.sum() == 198
        assert np.isnan(got.inverse[7]).all() and np.isnan(got.residual[11]) and got.samples[7] == 0


@pytest.mark.parametrize("sigma, angle", [(1.0, 0.0), (0.4, 0.3), (1.7, math.radians(30)), (3.3, -2.5), (7.9, math.pi)])
def test_planted_similarity_is_recovered(sigma, angle):
    template = fd.align_template(160, 0.1)
    planted = ao.inverse_of(sigma, angle, (311.5, 208.25), 160)
    got = fd.similarity_from_landmarks(ao.landmarks_of(planted, template)[None], template, 160)
    assert got.ok[0] and got.samples[0] in (ao.samples_of(sigma * (1 - 1e-9)), ao.samples_of(sigma * (1 + 1e-9)))
    assert np.allclose(got.inverse[0], planted, rtol=0, atol=1e-9)
    assert abs(got.scale[0] - 1 / sigma) < 1e-12 and got.residual[0] < 1e-12
    # the face is rolled by `angle` in the frame; the forward transform turns it back
    assert abs((got.angle[0] + math.degrees(angle) + 180) % 360 - 180) < 1e-9


def test_mirrored_points_still_give_a_proper_rotation():
    template = ao.align_template(112)
    mirrored = template * (-1, 1) * 2.0 + (400, 50)
    ref = ao.fit(mirrored, template)
    a, b = ref["forward"][:2]
    assert a * a + b * b > 0                                    # the determinant of [[a, -b], [b, a]]: never a reflection
    got = fd.similarity_from_landmarks(mirrored[None], template)
    assert got.ok[0] and got.scale[0] > 0 and got.inverse[0, 0] == got.inverse[0, 4] and got.inverse[0, 1] == -got.inverse[0, 3]
    assert got.residual[0] > 0.05                               # and the fit says so: the eyes cannot both land on the template


def test_alignable_rule():
    template = ao.align_template(112)

    def ok(points):
        got = fd.similarity_from_landmarks(np.asarray(points, np.float64)[None], template)
        assert bool(got.ok[0]) == ao.fit(points, template)["ok"]
        return bool(got.ok[0])
    assert ok(template) and ok(template * 3 + 17)
    assert not ok(np.full((5, 2), 33.0))                        # five coincident points: den = 0
    for bad in (np.nan, np.inf):
        points = template.copy()
        points[2, 1] = bad
        assert not ok(points)
    assert ok(template * 31.9) and not ok(template * 32.1)       # sigma = source pixels per output pixel: 1/16 .. 32
    assert ok(template / 15.9) and not ok(template / 16.1)
    assert ok(template + 1.6e7) and not ok(template + 1.7e7)     # an inverse entry of 2^24 or more


def test_template():
    assert np.allclose(fd.align_template(112, 0), np.asarray(fd.ARCFACE_112), rtol=0, atol=1e-12)
    assert fd.ARCFACE_112 == ao.ARCFACE_112 and fd.ARCFACE_112[2] == (56.0252, 71.7366)
    p = np.asarray(fd.ARCFACE_112)
    for size, margin in ((160, 0), (160, 0.25), (57, 0.14)):
        want = (p + 0.5 - 56) * (size / 112) / (1 + margin) + size / 2 - 0.5
        assert np.array_equal(fd.align_template(size, margin), want)
    # pixel centres scale, indices do not: the image centre stays the image centre, and a margin pulls the points towards it
    centre = fd.align_template(160, 0).mean(axis=0) - 79.5
    assert np.allclose(centre, (p.mean(axis=0) - 55.5) * 160 / 112)
    assert np.allclose(fd.align_template(160, 0.25) - 79.5, (fd.align_template(160, 0) - 79.5) / 1.25)


PILLOW_CASES = [((40, 56), (97, 131), (300, 400))[k % 3] + ((8, 57, 112, 160)[k % 4], (0.4, 1.0, 1.7, 3.3)[k // 3]) for k in range(12)]


def test_geometry_equals_pillows_affine_transform():
    """n = 1: floor of the unrounded value is Pillow's bilinear AFFINE transform (which maps pixel centres and truncates) at
    every pixel whose four taps lie inside the frame."""
    rng = np.random.default_rng(2)
    checked = differing = 0
    for h, w, size, sigma in PILLOW_CASES:
        frame = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        inv = ao.inverse_of(sigma, rng.uniform(-math.pi, math.pi), (rng.uniform(0.3, 0.7) * w, rng.uniform(0.3, 0.7) * h), size)
        c = inv[2] - 0.5 * (inv[0] + inv[1]) + 0.5
        f = inv[5] - 0.5 * (inv[3] + inv[4]) + 0.5
        pil = np.asarray(Image.fromarray(frame).transform((size, size), Image.AFFINE, (inv[0], inv[1], c, inv[3], inv[4], f), resample=Image.BILINEAR))
        inside = ao.interior(frame.shape, inv, size)
        mine = np.floor(ao.warp_values(frame, inv, 1, size)).astype(np.uint8)
        checked += int(inside.sum())
        differing += int((mine[inside] != pil[inside]).any(axis=-1).sum())
    print("interior pixels", checked, "differing", differing)
    assert checked > 20000 and differing == 0


def test_box_prefilter():
    rng = np.random.default_rng(3)
    frame = rng.integers(0, 256, (97, 131, 3), dtype=np.uint8)
    # sigma = 1, angle 0, an integer shift: a slice of the frame
    assert np.array_equal(ao.warp(frame, [1, 0, 11, 0, 1, 5], 1, 57), frame[5:62, 11:68])
    # a constant frame stays constant under the n = 3 prefilter wherever the footprint lies inside it
    flat = np.full((97, 131, 3), (77, 0, 255), np.uint8)
    inv = ao.inverse_of(2.6, 0.4, (65.0, 48.0), 16)
    out = ao.warp(flat, inv, 3, 16)
    assert (out == np.array((77, 0, 255), np.uint8)).all()
    # ... and it is the mean of the sub-samples: 2 x 2 samples at the centres of four source pixels
    assert np.array_equal(ao.warp(frame, [2, 0, 0.5, 0, 2, 0.5], 2, 8),
                          np.rint(frame[:16, :16].astype(np.float64).reshape(8, 2, 8, 2, 3).sum(axis=(1, 3)) / 4).astype(np.uint8))
    for sigma, n in ((1.0, 1), (1.0001, 2), (8.0, 8), (8.5, 8), (0.4, 1), (7.9, 8), (1.7, 2)):
        assert ao.samples_of(sigma) == n and fd.align_samples(np.array([sigma]))[0] == n


def test_arguments_are_checked_before_the_library(monkeypatch):
    def no_library():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "load", no_library)
    frame = np.zeros((16, 16, 3), np.uint8)

    def alignment(inverse, samples):
        count = len(samples)
        return fd.Alignment(np.asarray(inverse, np.float64), np.asarray(samples, np.int32), np.ones(count, bool),
                            np.zeros(count), np.ones(count), np.zeros(count))
    good = [1, 0, 0, 0, 1, 0]
    for inverse, samples, size in [([good], [1], 0), ([good], [1], 257), ([good], [0], 16), ([good], [9], 16), ([[1, 0, 2.0 ** 24, 0, 1, 0]], [1], 16),
                                   ([[1, 0, 0, math.nan, 1, 0]], [1], 16), ([[1, 0, 0, 0, math.inf, 0]], [1], 16), ([good[:5]], [1], 16),
                                   ([good, good], [1], 16), (np.zeros((0, 6)), [], 16), (np.tile(good, (65536, 1)), [1] * 65536, 16)]:
        with pytest.raises(ValueError):
            fd.align_faces(frame, alignment(inverse, samples), size)
    not_ok = fd.similarity_from_landmarks(np.full((1, 5, 2), 4.0), fd.align_template(16), 16)
    with pytest.raises(ValueError):
        fd.align_faces(frame, not_ok, 16)                        # a face that is not alignable cannot be warped


def test_workspace_entry_runs_on_the_host(lib):
    """fn_face_align_workspace needs no device: 6 doubles and one int32 per face, rounded up to 8 bytes; F outside 1 .. 65535 and
    a null result are the C ABI's argument error."""
    import ctypes as C
    nbytes = C.c_longlong(0)
    for F, want in ((1, 56), (2, 104), (3, 160), (65535, 65535 * 52 + 4)):
        assert lib.fn_face_align_workspace(F, C.byref(nbytes)) == 0 and nbytes.value == want
    for F in (0, -1, 65536):
        assert lib.fn_face_align_workspace(F, C.byref(nbytes)) == -1 and b"65535" in lib.fn_last_error()
    assert lib.fn_face_align_workspace(1, None) == -1


def test_bounding_box_without_landmarks_is_unchanged():
    box = fd.BoundingBox(61.4, 12.6, 20, 24, 0.6)
    assert (box.left, box.top, box.right, box.bottom, box.width, box.height, box.confidence) == (61, 13, 82, 38, 20, 24, 0.6)
    assert box.landmarks is None and box.info() == "[61, 13, 20, 24, 0.6]"
    marked = fd.BoundingBox(61.4, 12.6, 20, 24, 0.6, landmarks=np.arange(10).reshape(5, 2))
    assert marked.info() == box.info() and marked.landmarks.dtype == np.float32 and marked.landmarks.shape == (5, 2)
    assert fd.BoundingBox(1, 2, 3, 4).confidence is None


def test_pipeline_reads_the_align_key_and_drops_bad_fits(monkeypatch):
    make = lambda options, **kw: recognize.FacePipeline(SimpleNamespace(detect=lambda frame: ["a", "b", "c"]), None, options, device="cpu", **kw)
    assert not make(SimpleNamespace(size=160, margin=0)).align and not make(Config({"size": 160, "margin": 0})).align
    assert make(Config({"size": 160, "align": True})).align and not make(Config({"size": 160, "align": True}), align=False).align
    assert make(SimpleNamespace(size=160, margin=0), align=True).align

    crops = torch.arange(3, dtype=torch.uint8).reshape(3, 1, 1, 1).expand(3, 4, 4, 3)
    fits = fd.Alignment(np.zeros((3, 6)), np.ones(3, np.int32), np.array([True, True, False]), np.zeros(3), np.ones(3), np.array([0.01, 0.5, np.nan]))
    monkeypatch.setattr(recognize, "image_processing_aligned_batch", lambda frame, boxes, options: (crops, fits))
    frame = np.zeros((8, 8, 3), np.uint8)
    boxes, out = make(SimpleNamespace(size=4, margin=0), align=True).crops(frame)
    assert boxes == ["a", "b", "c"] and torch.equal(out, crops)
    boxes, out, kept = make(SimpleNamespace(size=4, margin=0), align=True, max_residual=0.1).aligned_crops(frame)
    assert boxes == ["a", "c"] and out[:, 0, 0, 0].tolist() == [0, 2] and kept.ok.tolist() == [True, False]
