"""fp64 references, derived error bounds, case inputs and fp32 restatements for the kernels of csrc/optim.hip: Adam
(fn_adam_keras, fn_adam_keras_ema), the step count (fn_adam_tick), the BatchNorm fold (fn_fold_bn) and the transposed pack
(fn_pack_transpose).  test_gpu_optim_edges.py compares the kernels with the references under the bounds; test_optim_refs_host.py
checks, without a GPU, that an fp32 restatement of each formula stays inside its bound on the same inputs and that planted errors
fall outside.  (The other update rules are restated bit for bit in tests/optimizer_oracle.py, the moving average in ema_oracle.py.)

Every bound has the project's form gamma_k absref (+ u_lp |ref| + eta_lp where the value is stored in 16 bits): k is the number of
fp32 roundings on the longest path, read off the kernel source and stated where the bound is built.  Every multiplication and
addition counts as rounded on its own (contraction to a fused multiply-add only removes roundings); sqrtf and / are one correctly
rounded operation each (hipcc's default, which the bit-exact fn_opt_keras tests rest on as well).  rsqrtf has no derivable
constant: it gets C_RSQRT ulps from elementwise_oracle, by the rule at the head of that file (4 x the error of the correctly
rounded fp32 restatement against fp64, at least 4 ulps); test_optim_refs_host.py measures that error on the fold's inputs:
0.50 ulp -> max(4, 4 x 0.50) = 4 = C_RSQRT.

The gamma model does not cover underflow, so every reference asserts that each of its intermediates is exactly zero or at least
2^-100 in magnitude (NO_UNDERFLOW).  Two places meet subnormals on purpose: beta2^t at t = 100000 is an fp32 subnormal, but it is
only an operand of fl(1 - beta2^t), and an fp32 addition of representable operands is exact-or-rounded whatever their size; and
the 16-bit packs may land in the f16 subnormal range, for which the bound carries eta_lp."""
import functools
from fractions import Fraction

import numpy as np
import torch

from tests.elementwise_oracle import BF, C_RSQRT, HF, _rsqrt32, lp_bound, lp_torch
from tests.util import U_FP32, gamma

U = U_FP32
F = np.float32
NO_UNDERFLOW = 2.0 ** -100

# ---------------------------------------------------------------------------------------------------------------------------
# Adam
# ---------------------------------------------------------------------------------------------------------------------------
LR, GS, BETA1, BETA2, EPS, L2, DECAY = 0.05, 0.5, 0.9, 0.999, 0.1, 5e-4, 0.9999
ADAM_N = 4096 + 8
# the L2 boundary: nowhere, everywhere, and inside a float4 at each of its three inner positions
ADAM_N_DECAY = (0, ADAM_N, 4 * 250 + 1, 4 * 500 + 2, 4 * 750 + 3)
ADAM_N_LP = (None, ADAM_N, 3560)                    # None: n_lp = 0 with w_lp = NULL
# 1101: beta1^t == 0 in fp32; 100000: beta2^t an fp32 subnormal; 10^6: both 0
ADAM_TS = (1, 2, 1000, 1101, 100_000, 10 ** 6)
ADAM_ZERO_SEGS = ((200, 264), (3600, 3664))         # w = g = m = v = 0: below every inner boundary and above it
ADAM_TIES = 3020                                    # start of the values that sit on the packs' rounding ties (g = m = 0 there)

GRID_CAP = 4096 * 256                               # float4s one trip of the optimiser kernels' grid-stride loop covers
STRIDE_N = 4 * (GRID_CAP + 257)
STRIDE_N_DECAY = 4 * (GRID_CAP + 100) + 1           # the L2 boundary and the end of the pack both lie in the second trip
STRIDE_N_LP = 4 * (GRID_CAP + 234)
STRIDE_ZERO_SEGS = ((4 * GRID_CAP + 40, 4 * GRID_CAP + 104), (4 * GRID_CAP + 940, 4 * GRID_CAP + 1004))
STRIDE_TIES = 4 * GRID_CAP + 420


def hyper_words(t, lr=LR, gs=GS, beta1=BETA1, beta2=BETA2):
    """The four fp32 words the kernel reads after the tick to step t (host mirror of fn_adam_tick)."""
    from facenet_amd.optimizers import adam_beta_powers
    b1t, b2t = adam_beta_powers(t, beta1, beta2)
    return np.array([lr, b1t, b2t, gs], dtype=F)


def tie_values():
    """fp32 values for the packs: exact bf16 ties (low half 0x8000) with an even and with an odd upper half, their neighbours
    0x7fff / 0x8001; exact f16 ties (low 13 bits 0x1000) over the f16 normal range and their neighbours; the f16 subnormal range:
    multiples and half-multiples of 2^-24, 2^-25 itself (tie to zero), values below it, and arbitrary values below 2^-14."""
    rng = np.random.default_rng(77)
    base = (rng.standard_normal(64) * 2.0).astype(F).view(np.uint32)
    out = []
    for low in (0x8000, 0x7FFF, 0x8001):
        out.append(((base & np.uint32(0xFFFF0000)) | np.uint32(low)).view(F))
    hb = (np.exp2(rng.uniform(-13.9, 15.9, 64)) * rng.choice([-1.0, 1.0], 64)).astype(F).view(np.uint32)
    for low in (0x1000, 0x0FFF, 0x1001):
        out.append(((hb & np.uint32(0xFFFFE000)) | np.uint32(low)).view(F))
    k = np.arange(1, 33, dtype=np.float64)
    sub = np.concatenate([k * 2.0 ** -24, (k + 0.5) * 2.0 ** -24, [2.0 ** -25, 2.0 ** -26, 3 * 2.0 ** -26, 1023.5 * 2.0 ** -24, 2.0 ** -14],
                          np.exp2(rng.uniform(-27, -14, 59))])
    out.append((sub * np.where(np.arange(sub.size) % 2, -1.0, 1.0)).astype(F))
    v = np.concatenate(out)
    assert np.all(np.isfinite(v)) and float(np.abs(v).max()) < 65504 and float(np.abs(v).min()) >= 2.0 ** -27
    return v


def _adam_inputs(n, zero_segs, ties_at, anchors, seed):
    rng = np.random.default_rng(seed)
    sign = lambda: rng.choice(np.array([-1.0, 1.0]), n)
    w = (sign() * np.power(10.0, rng.uniform(-2.0, 0.5, n))).astype(F)
    g = (sign() * np.power(10.0, rng.uniform(-6.0, 3.0, n))).astype(F)
    g[::17] = 0                                                  # exact zeros among the gradients
    m = (sign() * np.power(10.0, rng.uniform(-6.0, 0.0, n))).astype(F)
    v = np.power(10.0, rng.uniform(-12.0, 4.0, n)).astype(F)
    ties = tie_values()
    w[ties_at:ties_at + ties.size] = ties
    g[ties_at:ties_at + ties.size] = 0
    m[ties_at:ties_at + ties.size] = 0
    # the elements next to every inner L2 boundary are of moderate size, so that a boundary off by one moves them far outside
    for a in anchors:
        for i in (a - 1, a):
            w[i], g[i], m[i], v[i] = (1.25 if i % 2 else -1.25), 1e-2, 1e-3, 1e-4
    for lo, hi in zero_segs:
        for a in (w, g, m, v):
            a[lo:hi] = 0
    shadow = (w.astype(np.float64) + rng.standard_normal(n) * 0.1).astype(F)
    assert float(v.min()) >= 0
    return dict(w=w, g=g, m=m, v=v, shadow=shadow, n_ties=ties.size)


@functools.lru_cache(maxsize=None)
def adam_inputs():
    """fp32 w, g, m, v, shadow of the one-step cases (shared, never modified: callers copy)."""
    inp = _adam_inputs(ADAM_N, ADAM_ZERO_SEGS, ADAM_TIES, [d for d in ADAM_N_DECAY if 0 < d < ADAM_N], seed=5)
    assert ADAM_TIES + inp["n_ties"] <= min(x for x in ADAM_N_LP if x) and ADAM_TIES >= max(d for d in ADAM_N_DECAY if d < ADAM_N)
    return inp


@functools.lru_cache(maxsize=None)
def stride_inputs():
    """The same kinds of values over STRIDE_N elements, with the zero segments, the ties and the boundaries in the second trip."""
    return _adam_inputs(STRIDE_N, STRIDE_ZERO_SEGS, STRIDE_TIES, [STRIDE_N_DECAY], seed=6)


def assert_no_underflow(what, **arrays):
    for name, a in arrays.items():
        a = np.abs(np.asarray(a, dtype=np.float64))
        bad = (a != 0) & (a < NO_UNDERFLOW)
        assert not bad.any(), f"{what}: intermediate {name} in the underflow range at {int(bad.sum())} elements (min {a[bad].min():.3g})"


def adam_ref(w, g, m, v, hyper, n_decay, beta1=BETA1, beta2=BETA2, eps=EPS, l2=L2):
    """adam_keras_kernel in fp64 from the fp32 operands exactly as the kernel receives them (`hyper`: the fp32 words lr, beta1^t,
    beta2^t, grad_scale), with the bound of every output.  fp32 chain, one rounding per line unless stated:
        lr_t = lr * sqrtf(1 - b2t) / (1 - b1t)    1 - b2t; sqrtf (its argument's u counts half, rounded up to 1 with its own);
                                                  the product; 1 - b1t; the division: relative gamma_5
        p = g * gs;  q = (2 l2) * w  (2 l2 exact);  G = p + q on [0, n_decay), p elsewhere
                                                  every path to G: 2 roundings, over aG = |p| + |q| (the two may cancel)
        m' = beta1 * m + (1 - beta1) * G          1 - beta1; two products; the sum.  Paths: beta1 m: 2; the G term: 2 + 3
                                                  -> e_m = gamma_5 absref_m, absref_m = |beta1 m| + (1 - beta1) aG         k = 5
        v' = beta2 * v + ((1 - beta2) * G) * G    1 - beta2; three products; the sum.  Paths: beta2 v: 2; the G term: G twice
                                                  (2 + 2) + 4 -> e_v = gamma_8 absref_v, absref_v = beta2 v + (1 - beta2) aG^2   k = 8
        r = sqrtf(v')                             |sqrt(a) - sqrt(b)| <= min(|a - b| / sqrt(b), sqrt|a - b|), + u
        d = r + eps                               e_d = e_r + u (d + e_r)
        num = lr_t * m'                           e_num = |lr_t| (gamma_6 |m'| + (1 + gamma_6) e_m)      (gamma_5 of lr_t, the product)
        s = num / d                               e_s = (e_num + |s| e_d) / (d - e_d) + u (|s| + that)
        w' = w - s                                e_w = e_s + u (|w'| + e_s)
    Returns a dict of fp64 arrays m, v, w, e_m, e_v, e_w."""
    f64 = lambda x: float(np.float32(x))
    lr, b1t, b2t, gs = (float(np.float32(h)) for h in np.asarray(hyper)[:4])
    b1, b2, eps, l2 = f64(beta1), f64(beta2), f64(eps), f64(l2)
    w, g, m, v = (np.asarray(a, dtype=F).astype(np.float64) for a in (w, g, m, v))
    n = w.size
    decayed = np.arange(n) < n_decay
    p = g * gs
    q = np.where(decayed, 2.0 * l2 * w, 0.0)
    G, aG = p + q, np.abs(p) + np.abs(q)
    tm1, tm2 = b1 * m, (1.0 - b1) * G
    m1, abs_m = tm1 + tm2, np.abs(tm1) + (1.0 - b1) * aG
    e_m = gamma(5) * abs_m
    tv1, tv2 = b2 * v, (1.0 - b2) * G * G
    v1, abs_v = tv1 + tv2, np.abs(tv1) + (1.0 - b2) * aG * aG
    e_v = gamma(8) * abs_v
    one_b2t, one_b1t = 1.0 - b2t, 1.0 - b1t
    lr_t = lr * np.sqrt(one_b2t) / one_b1t
    r = np.sqrt(v1)
    with np.errstate(divide="ignore", invalid="ignore"):
        e_r = np.where(r > 0, np.minimum(e_v / r, np.sqrt(e_v)), np.sqrt(e_v))
    e_r = e_r + U * (r + e_r)
    d = r + eps
    e_d = e_r + U * (d + e_r)
    assert bool((e_d < 0.25 * d).all()), "denominator too ill-conditioned for a meaningful bound"
    num = lr_t * m1
    e_num = abs(lr_t) * (gamma(6) * np.abs(m1) + (1 + gamma(6)) * e_m)
    s = num / d
    e_s = (e_num + np.abs(s) * e_d) / (d - e_d)
    e_s = e_s + U * (np.abs(s) + e_s)
    w1 = w - s
    e_w = e_s + U * (np.abs(w1) + e_s)
    # b2t itself may be subnormal (an operand of an addition: see the head of the file); everything computed from it is checked
    assert_no_underflow("adam", p=p, q=q, G=G, tm1=tm1, tm2=tm2, m1=m1, tv1=tv1, tv2=tv2, v1=v1, one_b2t=one_b2t, one_b1t=one_b1t,
                        lr_t=lr_t, r=r, d=d, num=num, s=s, w1=w1, GG=(1.0 - b2) * G)
    return dict(m=m1, v=v1, w=w1, e_m=e_m, e_v=e_v, e_w=e_w)


def adam_f32(w, g, m, v, hyper, n_decay, beta1=BETA1, beta2=BETA2, eps=EPS, l2=L2, eps_inside_sqrt=False, bias_correction=True,
             square_g=True):
    """fp32 NumPy restatement of adam_keras_kernel, one rounding per operation, no fused multiply-add: (w', m', v').  The keyword
    arguments plant the errors the host test must see fall outside the bounds."""
    w, g, m, v = (np.asarray(a, dtype=F) for a in (w, g, m, v))
    lr, b1t, b2t, gs = (F(h) for h in np.asarray(hyper)[:4])
    b1, b2, eps, l2 = F(beta1), F(beta2), F(eps), F(l2)
    one = F(1.0)
    lr_t = lr * np.sqrt(one - b2t) / (one - b1t) if bias_correction else lr
    gg = g * gs
    gg[:n_decay] = gg[:n_decay] + (F(2.0) * l2) * w[:n_decay]
    m1 = b1 * m + (one - b1) * gg
    v1 = b2 * v + ((one - b2) * gg * gg if square_g else (one - b2) * gg)
    with np.errstate(invalid="ignore"):                # the unsquared gradient makes v' negative somewhere
        den = np.sqrt(v1 + eps) if eps_inside_sqrt else np.sqrt(v1) + eps
    return (w - lr_t * m1 / den).astype(F), m1.astype(F), v1.astype(F)


def pack_rne(w32, dt):
    """Round-to-nearest-even of fp32 values to the storage type: the int16 bit patterns (torch's CPU conversion is RNE, f16
    subnormals included)."""
    return torch.from_numpy(np.ascontiguousarray(w32, dtype=F)).to(lp_torch(dt)).view(torch.int16).numpy()


def pack_truncate(w32, dt):
    """The planted error: the same conversion by truncation of the magnitude (bf16: the upper half of the fp32 word)."""
    w32 = np.ascontiguousarray(w32, dtype=F)
    if dt == BF:
        return (w32.view(np.uint32) >> 16).astype(np.uint16).view(np.int16)
    rne = torch.from_numpy(w32).to(torch.float16)
    over = rne.float().abs() > torch.from_numpy(np.abs(w32))                     # rounded away from zero: step one f16 back
    bits = rne.view(torch.int16).numpy().copy()
    bits[over.numpy()] -= 1                                                      # sign-magnitude: one ulp towards zero
    return bits


def min_tie_distance(beta32, ts):
    """The smallest distance, in fp64 ulps of the power, of the exact rational float32(beta)^t (t in ts, ascending) from an
    fp32 rounding tie (a midpoint of two adjacent fp32 values, subnormals and zero included)."""
    b = Fraction(float(np.float32(beta32)))
    x, t_at, worst = Fraction(1), 0, None
    for t in ts:
        x *= b ** (t - t_at)
        t_at = t
        e = x.numerator.bit_length() - x.denominator.bit_length()        # 2^(e-1) <= x < 2^(e+1)
        if Fraction(2) ** e > x:
            e -= 1                                                        # 2^e <= x < 2^(e+1)
        spacing = Fraction(2) ** (max(e, -126) - 23)
        frac = x / spacing
        frac -= frac.numerator // frac.denominator                        # position inside the fp32 cell, in [0, 1)
        dist = abs(frac - Fraction(1, 2)) * spacing
        ulp64 = Fraction(2) ** (e - 52)
        d = dist / ulp64
        worst = d if worst is None or d < worst else worst
    return float(worst)


# ---------------------------------------------------------------------------------------------------------------------------
# layer tables (fn_fold_bn, fn_pack_transpose): rows {w_off, cout, ktot, taps, cin, bn_off, fold_bias_off, 0}
# ---------------------------------------------------------------------------------------------------------------------------
def make_table(shapes, first=16, gaps=(8, 24, 16)):
    """shapes: [(cout, taps, cin, bn_off, fb_off)] -> (int32 [L, 8], total elements): the layers at non-zero offsets that are
    multiples of 8, with a gap after each (and one past the last)."""
    tab = np.zeros((len(shapes), 8), dtype=np.int32)
    off = first
    for i, (cout, taps, cin, bn, fb) in enumerate(shapes):
        assert off % 8 == 0 and (cout * taps * cin) % 8 == 0
        tab[i] = [off, cout, taps * cin, taps, cin, bn, fb, 0]
        off += cout * taps * cin + gaps[i % len(gaps)]
    return tab, off


def covered(tab, total):
    """bool [total]: the elements that belong to a layer."""
    mask = np.zeros(total, dtype=bool)
    for off, cout, ktot in tab[:, :3]:
        assert not mask[off:off + cout * ktot].any()
        mask[off:off + cout * ktot] = True
    return mask


# ---------------------------------------------------------------------------------------------------------------------------
# fn_fold_bn
# ---------------------------------------------------------------------------------------------------------------------------
BN_EPS = 1e-3
# (cout, taps, cin, bn_off, fb_off): 8 vectors in all; 3x3x8; ktot 1792; no BatchNorm (weights merely rounded); BatchNorm
# without a folded bias; the fold_bias offsets differ from the bn offsets (the engine passes the same value for both words)
FOLD_SHAPES = [(8, 1, 8, 3, 40), (16, 9, 8, 13, 5), (24, 1, 1792, 31, 60), (8, 1, 128, -1, -1), (16, 9, 8, 57, -1), (40, 1, 72, 75, 90)]
FOLD_CB = 136                                       # channels of beta / mean / var / fold_bias: the layers' ranges leave gaps
FOLD_BIG = [(296, 1, 1792, 2, 2)]                   # 530,432 elements > 256 * 2048: past the grid cap of the stride loop
FOLD_BIG_CB = 304
K_FOLD_W = 1 + 2 * C_RSQRT + 1                      # fl(var + eps); rsqrtf: C_RSQRT ulps of <= 2u each; the product
K_FOLD_B = 1 + 2 * C_RSQRT + 1 + 1                  # ... the product mean * s; the subtraction


def fold_inputs(shapes, CB, seed=11):
    """(table, total, w fp32 [total], beta, mean, var fp32 [CB]).  Per channel, by its index in the layer modulo 4: variance 0,
    ~1, 1e-12 (eps dominates both small ones), 1e6 -- adjacent channels' scales differ by more than 2x, the wrap from the last
    channel class to the first included; every third channel's beta cancels mean * scale to within a few ulps."""
    tab, total = make_table(shapes)
    rng = np.random.default_rng(seed)
    w = (rng.standard_normal(total) * 0.1).astype(F)
    beta = (rng.standard_normal(CB) * 0.3).astype(F)
    mean = (rng.standard_normal(CB) * 3.0 + 5.0).astype(F)
    var = np.full(CB, 1.0, dtype=F)
    seen = np.zeros(CB, dtype=bool)
    for off, cout, ktot, taps, cin, bn, fb, _ in tab:
        if bn < 0:
            continue
        assert not seen[bn:bn + cout].any()
        seen[bn:bn + cout] = True
        co = np.arange(cout)
        var[bn:bn + cout] = np.choose(co % 4, [0.0, rng.uniform(0.5, 2.0, cout), 1e-12, 1e6]).astype(F)
        s = 1.0 / np.sqrt(var[bn:bn + cout].astype(np.float64) + float(F(BN_EPS)))
        ratio = np.maximum(s[1:] / s[:-1], s[:-1] / s[1:])
        assert float(ratio.min()) >= 2.0, "adjacent channels must differ in scale by at least 2x"
        ms = (mean[bn:bn + cout].astype(np.float64) * s).astype(F)
        near = ms.view(np.int32) + (co % 7 - 3).astype(np.int32)            # -3 .. +3 ulps from fl(mean * s)
        third = co % 3 == 0
        beta[bn:bn + cout][third] = near.view(F)[third]
    return tab, total, w, beta, mean, var


def fold_ref(tab, total, w, beta, mean, var, dt, eps=BN_EPS):
    """fold_bn_kernel in fp64: w / sqrt(var + eps) per out-channel and beta - mean / sqrt(var + eps), with bounds.
        t = fl(var + eps); s = rsqrtf(t)      relative gamma_{1 + 2 C_RSQRT} (the argument's u counts half)
        weight: round_lp(fl(w s))             u_lp |ref| + eta_lp + gamma_k |ref|, k = K_FOLD_W
        bias:   fl(beta - fl(mean s))         gamma_k absref, absref = |beta| + |mean s|, k = K_FOLD_B (fp32 output)
    A layer with bn < 0 has s = 1: its weights are the storage rounding of w, bit for bit (`exact` marks them).
    Returns (wf fp64 [total], bound [total], exact bool [total], fb fp64 [CB], fb_bound [CB], fb_covered bool [CB])."""
    eps = float(F(eps))
    w64 = np.asarray(w, dtype=F).astype(np.float64)
    beta, mean, var = (np.asarray(a, dtype=F).astype(np.float64) for a in (beta, mean, var))
    wf, exact = np.zeros(total), np.zeros(total, dtype=bool)
    fb, fb_abs, fb_cov = np.zeros(beta.size), np.zeros(beta.size), np.zeros(beta.size, dtype=bool)
    for off, cout, ktot, taps, cin, bn, fbo, _ in tab:
        sl = slice(off, off + cout * ktot)
        if bn < 0:
            wf[sl], exact[sl] = w64[sl], True
            continue
        t = var[bn:bn + cout] + eps
        s = 1.0 / np.sqrt(t)
        wf[sl] = (w64[sl].reshape(cout, ktot) * s[:, None]).reshape(-1)
        ms = mean[bn:bn + cout] * s
        assert_no_underflow("fold", t=t, s=s, ws=wf[sl], ms=ms, bias=beta[bn:bn + cout] - ms)
        if fbo >= 0:
            assert not fb_cov[fbo:fbo + cout].any()
            fb[fbo:fbo + cout] = beta[bn:bn + cout] - ms
            fb_abs[fbo:fbo + cout] = np.abs(beta[bn:bn + cout]) + np.abs(ms)
            fb_cov[fbo:fbo + cout] = True
    ref = torch.from_numpy(wf)
    bound = lp_bound(ref, ref.abs(), K_FOLD_W, dt).numpy()
    return wf, bound, exact, fb, gamma(K_FOLD_B) * fb_abs, fb_cov


def fold_f32(tab, total, w, beta, mean, var, dt, eps=BN_EPS, tail_from_next_channel=False, with_eps=True, minus=True):
    """fp32 restatement (1/sqrt correctly rounded, as _rsqrt32): (int16 bits of the pack [total], fold_bias fp32 [CB]); elements
    outside every layer are 0.  The keyword arguments plant errors: the scale of channel co + 1 on the last 8 elements of every
    channel; rsqrt(var) without eps; beta + mean * s."""
    w = np.asarray(w, dtype=F)
    out = np.zeros(total, dtype=F)
    fb = np.zeros(np.asarray(beta).size, dtype=F)
    for off, cout, ktot, taps, cin, bn, fbo, _ in tab:
        sl = slice(off, off + cout * ktot)
        if bn < 0:
            out[sl] = w[sl]
            continue
        t = var[bn:bn + cout].astype(F) + F(eps) if with_eps else var[bn:bn + cout].astype(F)
        with np.errstate(divide="ignore"):
            s = _rsqrt32(t)
        sc = np.repeat(s[:, None], ktot, axis=1)
        if tail_from_next_channel:
            sc[:-1, -8:] = s[1:, None]
        with np.errstate(invalid="ignore", over="ignore"):
            out[sl] = (w[sl].reshape(cout, ktot) * sc).reshape(-1)
            if fbo >= 0:
                ms = mean[bn:bn + cout].astype(F) * s
                fb[fbo:fbo + cout] = beta[bn:bn + cout].astype(F) - ms if minus else beta[bn:bn + cout].astype(F) + ms
    return torch.from_numpy(out).to(lp_torch(dt)).view(torch.int16).numpy(), fb


def lp_values(bits, dt):
    """int16 bit patterns of the storage type -> fp64 values."""
    return torch.from_numpy(np.ascontiguousarray(bits, dtype=np.int16)).view(lp_torch(dt)).double().numpy()


# ---------------------------------------------------------------------------------------------------------------------------
# fn_pack_transpose
# ---------------------------------------------------------------------------------------------------------------------------
# (cout, taps, cin): the 64 x 64 path with partial tiles on either side, one tile, many taps, and 168 tiles (more than the
# grid cap of 128) on the two 1792-wide layers; the scalar 32 x 32 path for cout % 8 != 0
TRANSPOSE_SHAPES = [(32, 9, 8), (80, 1, 64), (192, 9, 80), (8, 7, 128), (1792, 1, 384), (128, 1, 1792), (19, 1, 128), (37, 9, 40)]


def transpose_inputs():
    """(table, total, source int16 [total], sentinel int16 [total]).  i -> 40503 i + c is a bijection on 16 bits, so every
    window of 65536 elements holds every 16-bit pattern once (zeros, subnormals, infinities and NaNs of both types included)."""
    tab, total = make_table([(co, tp, ci, -1, -1) for co, tp, ci in TRANSPOSE_SHAPES])
    i = np.arange(total, dtype=np.int64)
    src = ((i * 40503 + 0x3A5C) & 0xFFFF).astype(np.uint16).view(np.int16)
    sentinel = ((i * 25173 + 0x1234) & 0xFFFF).astype(np.uint16).view(np.int16)
    return tab, total, src, sentinel


def transpose_ref(tab, src, sentinel, swap_tap_cin=False):
    """[cout][tap][cin] -> [cin][tap][cout] per layer, the sentinel everywhere else.  swap_tap_cin plants the error of reading
    the source as [cout][cin][tap]."""
    out = sentinel.copy()
    for off, cout, ktot, taps, cin, _, _, _ in tab:
        blk = src[off:off + cout * ktot]
        if swap_tap_cin:
            t = blk.reshape(cout, cin, taps).transpose(1, 2, 0)
        else:
            t = blk.reshape(cout, taps, cin).transpose(2, 1, 0)
        out[off:off + cout * ktot] = t.reshape(-1)
    return out


def table_preconditions(tab):
    """What the 16-byte paths of pack_transpose_kernel and fold_bn_kernel rely on, row by row; returns the offending rows."""
    tab = np.asarray(tab)
    bad = (tab[:, 0] % 8 != 0) | (tab[:, 4] % 8 != 0) | (tab[:, 1] % 8 != 0) | (tab[:, 2] != tab[:, 3] * tab[:, 4]) | (tab[:, 1] <= 0)
    return tab[bad]
