"""NumPy restatement of the training-time augmentation for one image and explicit per-image parameters:
rotate (bilinear, zero fill) -> crop or pad to S x S at signed offsets (y0, x0) -> horizontal flip.  float32 with the kernel's
operation order (every product and sum rounded on its own, no fused multiply-add), so fn_augment_u8 must match it bit for bit.
PARITY UNPINNED: the reference documents the config keys but has no implementation."""
import numpy as np

F = np.float32


def rotate(img: np.ndarray, cos_t, sin_t) -> np.ndarray:
    """R (the source's size) at every integer pixel: the bilinear sample of `img` at the rotated point, taps outside read 0."""
    h, w = img.shape[:2]
    c, s = F(cos_t), F(sin_t)
    hw2, hh2 = F(0.5) * F(w), F(0.5) * F(h)
    y, x = np.meshgrid(np.arange(h, dtype=F), np.arange(w, dtype=F), indexing="ij")
    u = (x + F(0.5)) - hw2
    v = (y + F(0.5)) - hh2
    sx = ((c * u - s * v) + hw2) - F(0.5)
    sy = ((s * u + c * v) + hh2) - F(0.5)
    flx, fly = np.floor(sx), np.floor(sy)
    x0, y0 = flx.astype(np.int64), fly.astype(np.int64)
    fx, fy = sx - flx, sy - fly
    gx, gy = F(1) - fx, F(1) - fy
    pad = np.zeros((h + 2, w + 2, 3), F)                  # one ring of zeros: taps at -1 .. h / w read 0
    pad[1:-1, 1:-1] = img

    def tap(yy, xx):
        inside = (yy >= -1) & (yy <= h) & (xx >= -1) & (xx <= w)
        v = pad[np.clip(yy + 1, 0, h + 1), np.clip(xx + 1, 0, w + 1)]
        return np.where(inside[..., None], v, F(0))

    gx, gy, fx, fy = (a[..., None] for a in (gx, gy, fx, fy))
    top = gx * tap(y0, x0) + fx * tap(y0, x0 + 1)
    bot = gx * tap(y0 + 1, x0) + fx * tap(y0 + 1, x0 + 1)
    val = gy * top + fy * bot
    assert val.dtype == F
    return np.clip(np.rint(val), 0, 255).astype(np.uint8)


def crop_or_pad(img: np.ndarray, size: int, y0: int, x0: int) -> np.ndarray:
    """C[y][x] = img[y + y0][x + x0] where that lies inside img, else 0."""
    h, w = img.shape[:2]
    out = np.zeros((size, size, 3), np.uint8)
    ys, xs = np.arange(size) + y0, np.arange(size) + x0
    my, mx = (ys >= 0) & (ys < h), (xs >= 0) & (xs < w)
    out[np.ix_(my, mx)] = img[np.ix_(ys[my], xs[mx])]
    return out


def augment(img: np.ndarray, size: int, y0: int, x0: int, flip, cos_t, sin_t) -> np.ndarray:
    r = img if (F(sin_t) == 0 and F(cos_t) == 1) else rotate(img, cos_t, sin_t)
    out = crop_or_pad(r, size, int(y0), int(x0))
    return out[:, ::-1].copy() if flip else out


def augment_batch(arrays, size: int, params) -> np.ndarray:
    """params: records with fields y0, x0, flip, cos, sin (facenet_amd.dataset.AUGMENT_PARAM)."""
    return np.stack([augment(a, size, p["y0"], p["x0"], p["flip"], p["cos"], p["sin"]) for a, p in zip(arrays, params)])
