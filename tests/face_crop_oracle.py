"""NumPy restatement of `PIL.Image.crop(window).resize((side, side), LANCZOS)` for 8-bit RGB (Pillow's Resample.c), the
semantics of fn_face_crop_resize_u8.  Pillow itself is the reference: tests/test_face_crop_host.py holds
this file to it bit for bit, and the GPU tests compare the kernel with Pillow directly.

Per axis (inSize -> side), all in float64: scale = inSize / side, fs = max(scale, 1), support = 3 * fs; for output index xx,
center = (xx + 0.5) * scale, xmin = max(int(center - support + 0.5), 0), n = min(int(center + support + 0.5), inSize) - xmin,
w[x] = L((x + xmin - center + 0.5) / fs) with L(t) = sinc(t) * sinc(t / 3) on [-3, 3), normalised by their left-to-right sum,
then fixed point k = int(w * 2^22 -+ 0.5) (truncation toward zero).  A pass is out = clamp((2^21 + sum k * pixel) >> 22, 0, 255)
stored as uint8; the horizontal pass runs first, the vertical one on its uint8 result, and an axis whose inSize == side is
copied."""
import math

import numpy as np

PRECISION_BITS = 22
MAX_SIDE = 256
MAX_EXTENT = 3072


def _sinc(t):
    if t == 0.0:
        return 1.0
    t = t * math.pi
    return math.sin(t) / t


def lanczos(t):
    return _sinc(t) * _sinc(t / 3) if -3.0 <= t < 3.0 else 0.0


def axis_taps(in_size: int, side: int):
    """-> (xmin int32 [side], n int32 [side], k int32 [side, kmax]) of one axis; the identity (in_size == side) is one tap of
    2^22 at the pixel itself, which the pass reproduces exactly."""
    if in_size == side:
        idx = np.arange(side, dtype=np.int32)
        return idx, np.ones(side, np.int32), np.full((side, 1), 1 << PRECISION_BITS, np.int32)
    scale = in_size / side
    fs = max(scale, 1.0)
    support = 3.0 * fs
    kmax = int(math.ceil(support)) * 2 + 1
    xmin, cnt, taps = np.zeros(side, np.int32), np.zeros(side, np.int32), np.zeros((side, kmax), np.int32)
    for xx in range(side):
        center = (xx + 0.5) * scale
        lo = max(int(center - support + 0.5), 0)
        n = min(int(center + support + 0.5), in_size) - lo
        w = [lanczos((x + lo - center + 0.5) / fs) for x in range(n)]
        ww = 0.0
        for v in w:
            ww += v
        for x, v in enumerate(w):
            if ww != 0.0:
                v = v / ww
            taps[xx, x] = int(v * (1 << PRECISION_BITS) - 0.5) if v < 0 else int(v * (1 << PRECISION_BITS) + 0.5)
        xmin[xx], cnt[xx] = lo, n
    return xmin, cnt, taps


def _pass(img, xmin, cnt, taps):
    """Resample axis 1 of uint8 [rows, in, 3] -> uint8 [rows, side, 3]."""
    out = np.empty((img.shape[0], len(xmin), 3), np.uint8)
    src = img.astype(np.int64)
    for xx in range(len(xmin)):
        k = taps[xx, :cnt[xx]].astype(np.int64)
        acc = (1 << (PRECISION_BITS - 1)) + np.tensordot(src[:, xmin[xx]:xmin[xx] + cnt[xx]], k, axes=([1], [0]))
        out[:, xx] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return out


def crop(frame, window):
    """PIL crop: uint8 [bottom - top, right - left, 3], zero outside the frame."""
    left, top, right, bottom = (int(v) for v in window)
    h, w = frame.shape[:2]
    out = np.zeros((bottom - top, right - left, 3), np.uint8)
    y0, y1, x0, x1 = max(top, 0), min(bottom, h), max(left, 0), min(right, w)
    if y1 > y0 and x1 > x0:
        out[y0 - top:y1 - top, x0 - left:x1 - left] = frame[y0:y1, x0:x1]
    return out


def crop_resize(frame, window, side):
    """uint8 [H, W, 3], (left, top, right, bottom), side -> uint8 [side, side, 3]."""
    img = crop(np.asarray(frame, np.uint8), window)
    ch, cw = img.shape[:2]
    img = _pass(img, *axis_taps(cw, side))                                       # horizontal first, stored as uint8
    return _pass(img.transpose(1, 0, 2), *axis_taps(ch, side)).transpose(1, 0, 2).copy()


def random_cases(count, seed=0):
    """The seeded case mix of the host test: (frame, window, side) with up- and down-scaling, non-square crops, windows that
    overhang every edge, identity on one or both axes and 0/255 frames that overshoot the clip on both sides."""
    rng = np.random.default_rng(seed)
    sides = (8, 24, 160, 182, 192)
    for i in range(count):
        h, w = int(rng.integers(20, 260)), int(rng.integers(20, 260))
        if i % 3 == 0:
            frame = (rng.integers(0, 2, (h, w, 3)) * 255).astype(np.uint8)
        else:
            frame = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        side = int(sides[i % len(sides)])
        cw, ch = int(rng.integers(1, 2 * w)), int(rng.integers(1, 2 * h))
        kind = i % 7
        if kind == 0:
            cw = side                                                             # horizontal pass skipped
        elif kind == 1:
            ch = side                                                             # vertical pass skipped
        elif kind == 2:
            cw = ch = side                                                        # pure copy
        elif kind == 3:
            cw, ch = int(rng.integers(4, 30)), int(rng.integers(4, 30))           # strong upscale
        left, top = int(rng.integers(-cw, w)), int(rng.integers(-ch, h))
        if kind == 4:
            left, top, cw, ch = -int(rng.integers(1, 9)), -int(rng.integers(1, 9)), w + 17, h + 13    # overhangs all four sides
        yield frame, (left, top, left + cw, top + ch), side
