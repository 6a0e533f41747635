"""The large-margin cosine softmax (NormFace / CosFace / ArcFace) in fp64, with per-element error bounds for
the three kernels of csrc/loss.hip (fn_margin_weight_rnorm, fn_margin_softmax_fwd_bwd, fn_margin_wgrad_fix), an fp32 restatement
in the kernels' order, and the input generator of the GPU and host tests.

The bounds are derived the way tests/elementwise_oracle.py derives softmax_ref's: every fp32 rounding of the kernel source is
counted (the kernels keep fused multiply-adds out, so the count is definite), errors of intermediate values are carried forward
as absolute bounds, and the two device functions without a published constant (__expf, logf) get elementwise_oracle's slack.
sqrtf and the division are correctly rounded: one rounding each."""
import math

import numpy as np
import torch

from oracle import facenet_oracle as fo
from tests.elementwise_oracle import ACC_GRAD_BITS, C_EXP, C_LOG, EXP_ARG_ULPS, U, cdiv, lp_torch
from tests.util import ETA_LP, U_LP, gamma

T_CLAMP = 1.0 - 2.0 ** -20
EPS = 1e-10
ETA_EXP = 2.0 ** -125             # __expf may flush a result below the smallest normal fp32 number (2^-126) to zero; x 2 for the shift of the maximum
MARGIN_GAP = 2.0 ** -10           # every target cosine that is no deliberate case keeps this distance from th and from +-T
SETTINGS = [(64.0, 0.5, 0.0), (30.0, 0.0, 0.35), (16.0, 0.0, 0.0)]      # ArcFace, CosFace, NormFace
SHAPES = [(6, 37, 40, 40), (90, 1000, 1000, 1008), (7, 8631, 8640, 8632)]


def f32(v):
    return float(np.float32(v))


def constants(m_arc):
    """(cos m2, sin m2, th, mm): in double from the fp32 value of m2, rounded to fp32 -- what the launch function passes on."""
    m = f32(m_arc)
    return f32(math.cos(m)), f32(math.sin(m)), f32(math.cos(math.pi - m)), f32(math.sin(math.pi - m) * m)


def rnd(val, err):
    """Error bound after one more fp32 rounding of a value known up to err."""
    return err + U * (val.abs() + err)


# ---------------------------------------------------------------------------------------------------------------------------
# fn_margin_weight_rnorm
# ---------------------------------------------------------------------------------------------------------------------------
def rnorm_ref(w, eps=EPS):
    """margin_rnorm_kernel: per lane 4 ceil(E / 256) products and adds in ascending e, 6 butterfly adds, the maximum with eps, a
    correctly rounded square root and a correctly rounded division.  Returns (r, bound)."""
    w = w.double()
    E = w.shape[1]
    eps = f32(eps)
    s = (w * w).sum(1)
    e_s = gamma(8 * cdiv(E, 256) + 6) * s
    t = s.clamp(min=eps)
    e_t = torch.where(s + e_s < eps, torch.zeros_like(s), e_s)          # clearly clamped rows: the argument is eps exactly
    r = t ** -0.5
    r_in = (t / (t - e_t)).sqrt() - 1
    r_r = (1 + r_in) * (1 + gamma(2)) - 1
    return r, r * r_r


def rnorm_f32(w, eps=EPS):
    f = np.float32
    w = w.numpy().astype(f)
    C, E = w.shape
    pad = np.zeros((C, cdiv(E, 256) * 256), f)
    pad[:, :E] = w
    trips = pad.reshape(C, -1, 64, 4)                                 # [trip][lane][element of the 16-byte load]
    s = np.zeros((C, 64), f)
    for k in range(trips.shape[1]):
        for t in range(4):
            s = s + trips[:, k, :, t] * trips[:, k, :, t]
    s = fo._wave_sum32(s)
    return torch.from_numpy(f(1.0) / np.sqrt(np.maximum(s, f(eps))))


def rnorm_inputs(C, E, seed):
    """fp32 [C, E] class rows at mixed scales with, when C >= 4: row 1 all zero (the eps branch), row 2 one-hot (r == 1 exactly)."""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(C, E, generator=g) * torch.logspace(-2, 1, C).view(C, 1)
    if C >= 4:
        w[1] = 0
        w[2] = 0
        w[2, E // 2] = -1.0
    return w


# ---------------------------------------------------------------------------------------------------------------------------
# fn_margin_softmax_fwd_bwd
# ---------------------------------------------------------------------------------------------------------------------------
def margin_inputs(N, C, ld, seed, m_arc):
    """z fp32 [N, ld] = c / r from chosen cosines, rnorm fp32 [ld], labels int32 [N]; padding columns of z and rnorm poisoned with
    1e30.  Rows (N >= 6): 0 -> label 0, a main-branch target; 1 -> label C - 1, a fallback target (ct <= th; only m_arc > 0 has a
    fallback above -T, otherwise a second main-branch target); 2 -> the class of row N - 1 (a repeated class), z r = 1.3: both clamps
    active, ct = T; 3 -> with m_arc > 0 the target exactly at ct == th (its r is 1.0 and z = th, the product is exact; it must take
    the fallback), otherwise z r = -1.3; 4 -> z r = -1.3 (ct = -T); the others draw a target cosine from (-0.95, 0.95).  Every
    target cosine that is none of the deliberate cases (rows 2, 3, 4) is at least MARGIN_GAP from th and from +-T: asserted."""
    assert N >= 6 and C >= 8
    g = torch.Generator().manual_seed(seed)
    th = constants(m_arc)[2]
    r = (0.5 + 1.5 * torch.rand(ld, generator=g)).float()
    labels = torch.randint(0, C, (N,), generator=g, dtype=torch.int32)
    labels[0], labels[1] = 0, C - 1
    labels[2] = labels[N - 1]
    at_th = m_arc > 0
    if at_th:
        r[int(labels[3])] = 1.0
    cos = (torch.rand(N, ld, generator=g) * 1.2 - 0.6).double()                  # the other classes: cosines in (-0.6, 0.6)
    tgt = torch.rand(N, generator=g).double() * 1.9 - 0.95
    near = (tgt - th).abs() < 4 * MARGIN_GAP
    tgt = torch.where(near, tgt + 8 * MARGIN_GAP, tgt)
    tgt[0] = 0.6
    tgt[1] = (th - T_CLAMP) / 2 if at_th else -0.7
    tgt[2], tgt[4] = 1.3, -1.3
    tgt[3] = th if at_th else -1.3
    rows = torch.arange(N)
    cos[rows, labels.long()] = tgt
    z = (cos / r.double()).float()
    if at_th:
        z[3, int(labels[3])] = th                                                   # r = 1: z r == th bit for bit
    z[:, C:] = 1e30
    r[C:] = 1e30
    c = (z.double() * r.double())[rows, labels.long()]
    free = torch.ones(N, dtype=torch.bool)
    free[[2, 3, 4]] = False
    for edge in (th, T_CLAMP, -T_CLAMP):
        assert bool(((c - edge).abs() >= MARGIN_GAP)[free].all()), "a target cosine too close to a branch or clamp edge"
    assert float(c[2]) > 1 and float(c[4]) < -1 and (float(c[3]) == th if at_th else float(c[3]) < -1)
    return z, r, labels


def margin_ref(z, rnorm, labels, C, scale, m_arc, m_cos, grad_scale, dt):
    """margin_softmax_kernel in fp64 with the error bound of every output.  z [N, >= C] and rnorm [>= C] are the kernel's own
    inputs (exact).  Roundings, as written in the kernel:
      c = clamp(fl(z r), -1, 1): one rounding unless the product is exact in fp32 or clearly clamped; the clamps are 1-Lipschitz, so they never grow an error.
      label column: ct = clamp(c, -T, T) (exact +-T when clearly clamped); a = fl(1 - ct), b = fl(1 + ct), q = fl(a b): three
      roundings on top of (2 |ct| + e) e from the error e of ct; sq = sqrtf(q): one; phi = fl(fl(fl(ct cos) - fl(sq sin)) - m3);
      D = fl(cos + fl(fl(ct sin) / sq)).  Fallback: phi = fl(fl(ct - mm) - m3), D = 1.
      l = fl(s c) or fl(s phi).  The kernel's maximum is the maximum of its own l, off by at most max e_l; softmax is invariant to
      that shift, so only the size of the exponent's argument feels it.  e_c = __expf(fl(l - mx)): the error of l and the rounded
      subtraction move the argument, then C_EXP + 1.45 |arg| ulps, and results below 2^-126 may be flushed (ETA_EXP).  The row sum,
      logf, 1 / s, and (p - onehot) grad_scale are softmax_ref's; then g = fl(fl(g0 s) D) (D == 1 multiplies exactly),
      dz = fl(g r) rounded once more to the storage type, t += fl(g c) converted to 2^-40 (half a unit per row).
    Returns a dict: loss, g, dz, t with e_*; the label column's q, phi, D with e_*; main (the branch); margin_ok (every branch and
    clamp decision of the label column is unambiguous in fp32)."""
    N = z.shape[0]
    cos_m, sin_m, th, mm = constants(m_arc)
    s_, m3, gs = f32(scale), f32(m_cos), f32(grad_scale)
    r = rnorm[:C].double().view(1, C)
    zs = z[:, :C].double()
    lab = labels.long().view(N, 1)
    craw = zs * r
    c = craw.clamp(-1.0, 1.0)
    exact = (craw.float().double() == craw) | (craw.abs() * (1 - U) >= 1)           # the fp32 product is exact, or clearly clamped
    e_c = torch.where(exact, torch.zeros_like(c), U * craw.abs())
    # ---- the label's column
    cl, e_cl = c.gather(1, lab), e_c.gather(1, lab)
    ct = cl.clamp(-T_CLAMP, T_CLAMP)
    e_ct = torch.where(cl.abs() - e_cl >= T_CLAMP, torch.zeros_like(ct), e_cl)
    main = ct > th
    at_edge = (ct == th) & (e_ct == 0)                                              # an exact product exactly at th: the fallback, decided
    margin_ok = bool((((ct - th).abs() > e_ct) | at_edge).all() and (((cl.abs() - T_CLAMP).abs() > e_cl) | (e_ct == 0)).all())
    a, b = 1 - ct, 1 + ct
    q = a * b
    dq = (2 * ct.abs() + e_ct) * e_ct
    k_q = torch.where(ct.abs() >= 0.5, 2.0, 3.0)                                    # 1 - |ct| is exact from 0.5 up (Sterbenz)
    e_q = dq + (k_q * U / (1 - k_q * U)) * (q + dq)
    sq = q.sqrt()
    e_sq = rnd(sq, sq - (q - e_q).clamp(min=0).sqrt())
    u_, v_, n_ = ct * cos_m, sq * sin_m, ct * sin_m
    e_u, e_v, e_n = rnd(u_, e_ct * abs(cos_m)), rnd(v_, e_sq * sin_m), rnd(n_, e_ct * sin_m)
    phi_main = u_ - v_ - m3
    e_phi_main = rnd(phi_main, rnd(u_ - v_, e_u + e_v))
    quot = n_ / sq
    e_quot = rnd(quot, (e_n * sq + n_.abs() * e_sq) / (sq * (sq - e_sq)))
    D_main = cos_m + quot
    e_D_main = rnd(D_main, e_quot)
    phi_fb = ct - mm - m3
    e_phi_fb = rnd(phi_fb, rnd(ct - mm, e_ct))
    phi = torch.where(main, phi_main, phi_fb)
    e_phi = torch.where(main, e_phi_main, e_phi_fb)
    D = torch.where(main, D_main, torch.ones_like(ct))
    e_D = torch.where(main, e_D_main, torch.zeros_like(ct))
    # ---- logits, softmax, loss
    onehot = torch.zeros_like(zs).scatter_(1, lab, 1.0)
    l = s_ * c
    e_l = rnd(l, s_ * e_c)
    l = l.scatter(1, lab, s_ * phi)
    e_l = e_l.scatter(1, lab, rnd(s_ * phi, s_ * e_phi))
    mx = l.max(1, keepdim=True).values
    e_mx = e_l.max(1, keepdim=True).values
    A = (l - mx).abs() + e_l + e_mx                                                 # size of the exponent's argument
    e = (l - mx).exp()
    r_e = (e_l + U * A).exp() * (1 + 2 * U * (C_EXP + EXP_ARG_ULPS * A * (1 + U))) - 1
    de = e * r_e + ETA_EXP
    ks = cdiv(C, 256) + 6 + 3
    ssum = e.sum(1, keepdim=True)
    e_s = de.sum(1, keepdim=True) * (1 + gamma(ks)) + gamma(ks) * ssum
    r_s = e_s / ssum
    r_inv = r_s / (1 - r_s)
    lse = ssum.log()
    xl, e_xl = l.gather(1, lab), e_l.gather(1, lab)
    e_log = r_inv + 2 * C_LOG * U * (lse.abs() + e_mx + r_inv)
    full = lse + mx
    e_full = rnd(full, e_log)
    row = full - xl
    e_row = rnd(row, e_full + e_xl)
    loss = row.sum() / N
    e_rows = (rnd(row / N, e_row / N) + 2.0 ** -(ACC_GRAD_BITS + 1)).sum()
    e_loss = e_rows + U * (loss.abs() + e_rows)                                     # acc_get rounds the total to fp32
    p = e / ssum
    e_p = (de / ssum + p * r_inv) * (1 + gamma(2)) + gamma(2) * p                   # e_c, 1 / s (its own rounding), the product
    g0 = (p - onehot) * gs
    e_g0 = rnd(g0, rnd(p - onehot, e_p) * abs(gs))
    g1 = g0 * s_
    e_g1 = rnd(g1, e_g0 * s_)
    Dfull = torch.ones_like(zs).scatter(1, lab, D)
    g = g1 * Dfull
    e_gl = rnd(g.gather(1, lab), e_g1.gather(1, lab) * (D + e_D) + g1.gather(1, lab).abs() * e_D)
    e_g = e_g1.scatter(1, lab, e_gl)
    dz = g * r
    e_dz32 = rnd(dz, e_g * r)
    e_dz = e_dz32 + U_LP[dt] * (dz.abs() + e_dz32) + ETA_LP[dt]
    term = g * c
    e_term = rnd(term, e_g * (c.abs() + e_c) + g.abs() * e_c) + 2.0 ** -(ACC_GRAD_BITS + 1)
    return dict(loss=loss, e_loss=e_loss, g=g, e_g=e_g, dz=dz, e_dz=e_dz, t=term.sum(0), e_t=e_term.sum(0), c=c, p=p,
                q=q, e_q=e_q, phi=phi, e_phi=e_phi, D=D, e_D=e_D, main=main, margin_ok=margin_ok)


def margin_f32(z, rnorm, labels, C, scale, m_arc, m_cos, grad_scale, dt, plant=None):
    """fp32 restatement in the kernel's order (256 threads striding the columns, wave butterflies, 4 wave totals), with a correctly
    rounded fp32 exp and log.  plant: one deliberate error -- 'ge' (>= instead of > at th), 'no_D' (dphi/dc left out), 'no_r' (r left
    out of dz), 't_no_c' (t summed without c), 'sub' (1 - ct^2 by subtraction).  Returns loss, dz (storage type), t (int64), extras."""
    f = np.float32
    N = z.shape[0]
    cos_m, sin_m, th, mm = (f(v) for v in constants(m_arc))
    s_, m3, gs, Tc = f(scale), f(m_cos), f(grad_scale), f(T_CLAMP)
    r = rnorm[:C].numpy().astype(f)[None, :]
    zs = z[:, :C].numpy().astype(f)
    lab = labels.long().numpy()
    rows = np.arange(N)
    c = np.minimum(np.maximum(zs * r, f(-1)), f(1))
    ct = np.minimum(np.maximum(c[rows, lab], -Tc), Tc)
    main = (ct >= th) if plant == "ge" else (ct > th)
    a, b = f(1) - ct, f(1) + ct
    q = (f(1) - ct * ct) if plant == "sub" else a * b
    sq = np.sqrt(q)
    with np.errstate(divide="ignore", invalid="ignore"):
        phi_main = ((ct * cos_m) - (sq * sin_m)) - m3
        D_main = cos_m + (ct * sin_m) / sq
    phi = np.where(main, phi_main, (ct - mm) - m3).astype(f)
    D = np.where(main, D_main, f(1)).astype(f)
    if plant == "no_D":
        D = np.ones_like(D)
    l = s_ * c
    l[rows, lab] = s_ * phi
    mx = l.max(1, keepdims=True)
    arg = l - mx
    e = np.exp(arg.astype(np.float64)).astype(f)
    pad = np.zeros((N, cdiv(C, 256) * 256), f)
    pad[:, :C] = e
    th_ = pad.reshape(N, -1, 256)
    acc = np.zeros((N, 256), f)
    for t in range(th_.shape[1]):
        acc = acc + th_[:, t]
    w = fo._wave_sum32(acc.reshape(N, 4, 64))
    ssum = ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]
    lse = np.log(ssum.astype(np.float64)).astype(f)
    rws = ((lse + mx[:, 0]) - l[rows, lab]) / f(N)
    loss = f(float(np.rint(rws.astype(np.float64) * 2.0 ** ACC_GRAD_BITS).astype(np.int64).sum()) * 2.0 ** -ACC_GRAD_BITS)
    inv = f(1) / ssum
    onehot = np.zeros_like(zs)
    onehot[rows, lab] = 1
    g = ((e * inv[:, None] - onehot) * gs) * s_
    g[rows, lab] = g[rows, lab] * D
    dz = g if plant == "no_r" else g * r
    term = g if plant == "t_no_c" else g * c
    t = np.rint(term.astype(np.float64) * 2.0 ** ACC_GRAD_BITS).astype(np.int64).sum(0)
    return loss, torch.from_numpy(dz).to(lp_torch(dt)), torch.from_numpy(t), dict(q=q, phi=phi, D=D, g=g, main=main)


# ---------------------------------------------------------------------------------------------------------------------------
# fn_margin_wgrad_fix and the whole gradient
# ---------------------------------------------------------------------------------------------------------------------------
def wgrad_fix_ref(dw, w, rnorm, t_acc):
    """margin_wgrad_fix_kernel: tf = fl(t 2^-40), k = fl(fl(r r) tf), dw - fl(k w): four roundings of the product, one of the
    difference.  dw, w fp32 [C, E]; rnorm fp32 [C]; t_acc int64 [C].  Returns (ref, bound)."""
    r = rnorm.double().view(-1, 1)
    t = t_acc.double().view(-1, 1) * 2.0 ** -ACC_GRAD_BITS
    prod = r * r * t * w.double()
    ref = dw.double() - prod
    return ref, rnd(ref, gamma(4) * prod.abs())


def wgrad_fix_f32(dw, w, rnorm, t_acc):
    f = np.float32
    r = rnorm.numpy().astype(f)[:, None]
    tf = (t_acc.numpy().astype(np.float64) * 2.0 ** -ACC_GRAD_BITS).astype(f)[:, None]
    k = (r * r) * tf
    return torch.from_numpy(dw.numpy().astype(f) - k * w.numpy().astype(f))


def wgrad_fix_inputs(C, E, seed, rows=None):
    """dw, w fp32 [rows >= C, E], rnorm fp32 [C] (as fn_margin_weight_rnorm defines it, correctly rounded), t int64 [C]."""
    g = torch.Generator().manual_seed(seed)
    rows = rows or C
    w = torch.randn(rows, E, generator=g) * 0.3
    dw = torch.randn(rows, E, generator=g) * 1e-2
    rnorm = (w[:C].double().pow(2).sum(1).clamp(min=EPS) ** -0.5).float()
    t = (torch.randn(C, generator=g).double() * 0.05 * 2.0 ** ACC_GRAD_BITS).round().to(torch.int64)
    return dw, w, rnorm, t


def head_fp64(xn, W, labels, scale, m_arc, m_cos):
    """The whole head in fp64 from the normalised embedding xn [N, E] and the class rows W [C, E], by the definition (straight-
    through clamps, dphi/dc at ct, the constants rounded to fp32): loss, dW = dz^T xn - r^2 t w, dxn = dz W."""
    xn, W = xn.double(), W.double()
    N, C = xn.shape[0], W.shape[0]
    r = (W * W).sum(1).clamp(min=f32(EPS)) ** -0.5
    z = xn @ W.t()
    o = margin_ref(z, r, labels, C, scale, m_arc, m_cos, 1.0 / N, 0)
    # margin_ref rounds scale, m_cos and grad_scale to fp32 as the kernel's arguments are: 1 / N is taken back out exactly
    g = o["g"] / f32(1.0 / N) / N
    dz = g * r.view(1, C)
    t = (g * o["c"]).sum(0)
    dW = dz.t() @ xn - (r * r * t).view(C, 1) * W
    return o["loss"], dW, dz @ W
