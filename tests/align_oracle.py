"""The definition of landmark alignment, NumPy float64: the five-point template, the closed-form
least-squares similarity from a face's landmarks onto it, the rule for when a face is alignable, and the warp that
fn_face_align_u8 computes (bilinear taps with a constant-zero border under an n x n box prefilter).  The GPU tests compare the
kernel with `warp` bit for bit; tests/test_align_host.py pins the fit against numpy.linalg.lstsq and the warp's geometry against
Pillow's affine transform.

Everything is fp64 in exactly the order written here: NumPy multiplies and adds in separate steps, so nothing is fused."""
import math

import numpy as np

ARCFACE_112 = ((38.2946, 51.6963), (73.5318, 51.5014), (56.0252, 71.7366), (41.5493, 92.3655), (70.7299, 92.2041))
SIGMA_MIN, SIGMA_MAX, ENTRY_MAX, MAX_SAMPLES = 1 / 16, 32.0, float(1 << 24), 8


def align_template(size, margin=0):
    """float64 [5, 2] (x, y), pixel-index coordinates of a size x size image: the pixel CENTRES of the 112 template scale about
    the image centre, and `margin` shrinks the face as the box path's relative margin does."""
    p = np.asarray(ARCFACE_112, np.float64)
    return (p + 0.5 - 56) * (size / 112) / (1 + margin) + size / 2 - 0.5


def samples_of(sigma):
    return min(MAX_SAMPLES, max(1, math.ceil(sigma)))


def fit(landmarks, template, size=112):
    """One face: float [5, 2] landmarks, float64 [5, 2] template -> dict(ok, forward (a, b, tx, ty), inverse [6], samples, sigma,
    angle, scale, residual).  A face that is not alignable has ok False and nothing else of meaning."""
    p = [(float(x), float(y)) for x, y in np.asarray(landmarks, np.float64)]
    q = [(float(x), float(y)) for x, y in np.asarray(template, np.float64)]
    bad = {"ok": False, "inverse": [math.nan] * 6, "samples": 0, "angle": math.nan, "scale": math.nan, "residual": math.nan}
    if not all(math.isfinite(c) for pt in p for c in pt):
        return bad
    pmx, pmy = sum(x for x, _ in p) / 5, sum(y for _, y in p) / 5
    qmx, qmy = sum(x for x, _ in q) / 5, sum(y for _, y in q) / 5
    den = dot = cross = 0.0
    for (px, py), (qx, qy) in zip(p, q):
        px, py, qx, qy = px - pmx, py - pmy, qx - qmx, qy - qmy
        den += px * px + py * py
        dot += px * qx + py * qy
        cross += px * qy - py * qx
    if not (math.isfinite(den) and den > 0):
        return bad
    a, b = dot / den, cross / den
    tx, ty = qmx - (a * pmx - b * pmy), qmy - (b * pmx + a * pmy)
    d = a * a + b * b
    if not (math.isfinite(d) and d > 0):
        return bad
    ia, ib = a / d, -b / d
    inverse = [ia, -ib, -(ia * tx - ib * ty), ib, ia, -(ib * tx + ia * ty)]
    sigma = 1 / math.sqrt(d)
    if not (SIGMA_MIN <= sigma <= SIGMA_MAX and all(math.isfinite(e) and abs(e) < ENTRY_MAX for e in inverse)):
        return bad
    sq = 0.0
    for (px, py), (qx, qy) in zip(p, q):
        ex, ey = (a * px - b * py) + tx - qx, (b * px + a * py) + ty - qy
        sq += ex * ex + ey * ey
    return {"ok": True, "forward": (a, b, tx, ty), "inverse": inverse, "samples": samples_of(sigma), "sigma": sigma,
            "angle": math.degrees(math.atan2(b, a)), "scale": math.sqrt(d), "residual": math.sqrt(sq / 5) / size}


def warp_values(frame, inverse, samples, size):
    """uint8 [H, W, 3], the six inverse entries, n, S -> float64 [S, S, 3]: the mean of the n x n sub-samples, unrounded."""
    frame = np.asarray(frame)
    H, W = frame.shape[:2]
    src = frame.astype(np.float64)
    inv = [float(e) for e in inverse]
    n = int(samples)
    v, u = np.meshgrid(np.arange(size, dtype=np.float64), np.arange(size, dtype=np.float64), indexing="ij")
    acc = np.zeros((size, size, 3), np.float64)

    def tap(xi, yi):
        inside = (xi >= 0) & (xi < W) & (yi >= 0) & (yi < H)
        return np.where(inside[..., None], src[np.clip(yi, 0, H - 1), np.clip(xi, 0, W - 1)], 0.0)

    for j in range(n):
        vv = v + ((j + 0.5) / n - 0.5)
        for i in range(n):
            uu = u + ((i + 0.5) / n - 0.5)
            x = (inv[0] * uu + inv[1] * vv) + inv[2]
            y = (inv[3] * uu + inv[4] * vv) + inv[5]
            xf, yf = np.floor(x), np.floor(y)
            fx, fy = (x - xf)[..., None], (y - yf)[..., None]
            x0, y0 = xf.astype(np.int64), yf.astype(np.int64)
            top = tap(x0, y0) * (1 - fx) + tap(x0 + 1, y0) * fx
            bot = tap(x0, y0 + 1) * (1 - fx) + tap(x0 + 1, y0 + 1) * fx
            acc += top * (1 - fy) + bot * fy
    return acc / (n * n)


def warp(frame, inverse, samples, size):
    """-> uint8 [S, S, 3]: `warp_values` rounded half to even."""
    return np.clip(np.rint(warp_values(frame, inverse, samples, size)), 0, 255).astype(np.uint8)


def interior(frame_shape, inverse, size):
    """bool [S, S]: the output pixels whose four taps at n = 1 lie inside the frame."""
    H, W = frame_shape[:2]
    inv = [float(e) for e in inverse]
    v, u = np.meshgrid(np.arange(size, dtype=np.float64), np.arange(size, dtype=np.float64), indexing="ij")
    x0 = np.floor((inv[0] * u + inv[1] * v) + inv[2])
    y0 = np.floor((inv[3] * u + inv[4] * v) + inv[5])
    return (x0 >= 0) & (x0 + 1 < W) & (y0 >= 0) & (y0 + 1 < H)


def inverse_of(sigma, angle, centre, size):
    """The six inverse entries of the similarity that puts the frame point `centre` = (x, y) at the output's centre with
    `sigma` source pixels per output pixel, the face rolled by `angle` radians: for planting test cases."""
    c, s = sigma * math.cos(angle), sigma * math.sin(angle)
    m = (size - 1) / 2
    return [c, -s, centre[0] - (c * m - s * m), s, c, centre[1] - (s * m + c * m)]


def landmarks_of(inverse, template):
    """The frame landmarks that the inverse transform sends the template's points to: float64 [5, 2]."""
    q = np.asarray(template, np.float64)
    i0, i1, i2, i3, i4, i5 = (float(e) for e in inverse)
    return np.stack([i0 * q[:, 0] + i1 * q[:, 1] + i2, i3 * q[:, 0] + i4 * q[:, 1] + i5], axis=1)
