"""fp64 references, derived error bounds, case inputs and fp32 restatements for the kernels of csrc/elementwise.hip and
csrc/loss.hip.  The GPU edge tests (test_gpu_elementwise_edges.py, test_gpu_loss_edges.py) compare the kernels with the
references under the bounds; test_elementwise_refs_host.py checks, without a GPU, that an fp32 restatement of each formula stays
inside its bound on the same inputs and that a planted error falls outside.

Every bound has the project's form u_lp |ref| + gamma_k absref (+ eta): k is the number of fp32 roundings in the longest chain,
read off the kernel source and stated where the bound is built.  Three device functions have no derivable constant (rsqrtf,
__expf, logf); they get a slack of C_* fp32 ulps, fixed here and justified by the host test (4 x the error of a correctly
rounded fp32 restatement against fp64, at least 4)."""
import math

import numpy as np
import torch

from oracle import facenet_oracle as fo
from tests.util import ETA_LP, U_FP32, U_LP, gamma

U = U_FP32
BF, HF = 0, 1                      # FN_BF16, FN_F16
ACC_STAT_BITS, ACC_GRAD_BITS = 20, 40

# ulp slack of the device functions without a published bound.  test_elementwise_refs_host.py measures the error of the correctly
# rounded fp32 restatement against fp64 on the GPU cases' inputs: rsqrt 0.50 ulp, exp 0.50 ulp (+ the argument term), log 0.50 ulp
# -> c = max(4, 4 * measured) = 4 for each.  One fp32 ulp is at most 2u relative.
C_RSQRT, C_EXP, C_LOG = 4, 4, 4
EXP_ARG_ULPS = 1.45                # __expf(x) = exp2(fl(x * log2 e)): the rounded product moves the result by <= 1.45 |x| ulps


def lp_torch(dt):
    return torch.bfloat16 if dt == BF else torch.float16


def cdiv(a, b):
    return (a + b - 1) // b


def ulps(got, ref):
    """|got - ref| in units of the fp32 ulp of ref (fp64 arrays)."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    e = np.floor(np.log2(np.maximum(np.abs(ref), 2.0 ** -126)))
    return np.abs(got - ref) / 2.0 ** (e - 23)


def check_bound(got, ref, bound, what):
    """|got - ref| <= bound at EVERY element (fp64 tensors); NaN fails."""
    got, ref, bound = (torch.as_tensor(v).double().cpu() for v in (got, ref, bound))
    bound = bound.expand_as(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = (got - ref).abs()
    bad = ~(err <= bound)
    if bool(bad.any()):
        excess = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err - bound)
        i = int(excess.reshape(-1).argmax())
        idx = tuple(int(v) for v in np.unravel_index(i, tuple(got.shape)))
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements outside the bound; worst at {idx}: got "
                             f"{float(got[idx]):.9g}, fp64 {float(ref[idx]):.9g}, |err| {float(err[idx]):.3g} > bound {float(bound[idx]):.3g}")


def inside(got, ref, bound):
    got, ref, bound = (torch.as_tensor(v).double() for v in (got, ref, bound))
    return bool(((got - ref).abs() <= bound).all())


def lp_bound(ref, absref, k, dt):
    """The bound assert_elementwise applies, as a tensor: u_lp (|ref| + gamma_k absref) + gamma_k absref + eta."""
    g = gamma(k)
    return U_LP[dt] * (ref.abs() + g * absref) + g * absref + ETA_LP[dt]


# ---------------------------------------------------------------------------------------------------------------------------
# BatchNorm (+ReLU), training
# ---------------------------------------------------------------------------------------------------------------------------
# (name, M, C, c0, ld_y, ld_z, replicas, relu, moving statistics, reduced, far)   ld_z is also the stride of dz
def bn_cases():
    out = []
    # last-stripe widths 1..8 in this order (ncg = 3, 5, 6, 7 leave idle tx lanes, ncg = 1 gives TY = 256 and 8 LDS fold passes),
    # then 72 = one full stripe + one group
    for i, C in enumerate([8, 16, 24, 32, 104, 48, 120, 192, 72]):
        w = ((C - 1) % 64) // 8 + 1
        out.append((f"width{w}_C{C}_whole_reps{(1, 3, 7)[i % 3]}", 300, C, 0, C, C, (1, 3, 7)[i % 3], 1, True, 0, False))
        out.append((f"width{w}_C{C}_slice_reps{(3, 7, 1)[i % 3]}", 300, C, 8 * (1 + i % 2), C + 24, C + 40, (3, 7, 1)[i % 3], i % 2, i % 2 == 0, 1,
                    False))
    out.append(("rows5_one_short_chunk", 5, 72, 0, 72, 72, 1, 1, True, 0, False))
    out.append(("rows33_second_chunk_of_one_row", 33, 72, 16, 96, 104, 3, 0, False, 0, False))
    # M * stripes = 70000 > 65536: the forward / apply kernels get rows_per_block = 35 (rr >= r1 inside a four-row trip), the
    # reduce kernel 139 rows per block
    out.append(("rows5000_rpb35", 5000, 896, 0, 896, 896, 7, 1, True, 0, False))
    out.append(("mean_far_from_zero", 300, 64, 0, 64, 64, 1, 1, True, 1, True))
    return out


def bn_inputs(dt, M, C, seed, far=False):
    """CPU tensors: y, dz (storage type), beta (fp32), exact fixed-point sums S1, S2 (int64, ACC_STAT_BITS)."""
    g = torch.Generator().manual_seed(seed)
    if far:         # the data of test_batchnorm_statistics_with_mean_far_from_zero: |mean| = 50 std on half of the channels
        ratio = torch.tensor([50.0] * (C // 2) + [0.0] * (C - C // 2))
        std = torch.tensor([1.0] * (C // 4) + [0.05] * (C // 4) + [0.25] * (C - 2 * (C // 4)))
        y = torch.randn(M, C, generator=g) * std + ratio * std
    else:
        y = torch.randn(M, C, generator=g) * 2.0 + torch.randn(C, generator=g)
    y = y.to(lp_torch(dt))
    dz = torch.randn(M, C, generator=g).to(lp_torch(dt))
    beta = torch.randn(C, generator=g) * 0.3
    y64 = y.double()
    S1 = (y64.sum(0) * 2.0 ** ACC_STAT_BITS).round().to(torch.int64)
    S2 = ((y64 * y64).sum(0) * 2.0 ** ACC_STAT_BITS).round().to(torch.int64)
    return y, dz, beta, S1, S2


def split_replicas(S, reps, seed):
    """int64 [reps, C] with uneven, partly negative parts whose exact integer sum is S."""
    g = torch.Generator().manual_seed(seed)
    parts = torch.randint(-(1 << 34), 1 << 34, (reps, S.numel()), generator=g, dtype=torch.int64)
    parts[reps - 1] = S - parts[:reps - 1].sum(0)
    assert torch.equal(parts.sum(0), S)
    return parts


def acc_buffer(parts1, parts2, C, sq_off, stride, junk=0x5A5A5A5A5A5A):
    """[reps * stride] int64: replica r holds parts1[r] at r*stride and parts2[r] at r*stride + sq_off; every other word is junk a
    kernel that reads outside its columns would pick up."""
    reps = parts1.shape[0]
    buf = torch.full((reps, stride), junk, dtype=torch.int64)
    buf[:, :C] = parts1
    buf[:, sq_off:sq_off + C] = parts2
    return buf.reshape(-1)


def bn_affine_ref(S1, S2, M, eps, beta, bits=ACC_STAT_BITS):
    """common.h bn_affine_from_sums in fp64 from the exact integer sums, with the error bound of every output, operation by
    operation (contraction is off there, so each line is one rounding):
        s1f = fl(S1 2^-bits), s2f likewise       rel u each (acc_get: exact in double, rounded once)
        inv = fl(1 / M)                          rel u
        mean = fl(s1f inv)                       rel gamma_3
        ex2 = fl(s2f inv)                        rel gamma_3
        m2 = fl(mean mean)                       rel gamma_7
        var = max(fl(ex2 - m2), 0)               abs gamma_3 ex2 + gamma_7 m2, + u on the result: the cancellation term
        t = fl(var + eps)                        abs e_var + u t
        scale = rsqrtf(t)                        rel sqrt(t / (t - e_t)) - 1 from the argument, + C_RSQRT ulps of the function
        ms = fl(mean scale)                      rel gamma_3, scale's, + u
        shift = fl(beta - ms)                    abs e_ms + u |shift|
    Returns fp64 tensors: scale, shift, mean, var and e_scale, e_shift, e_mean, e_var."""
    assert int(S1.abs().max()) < 1 << 53 and int(S2.abs().max()) < 1 << 53          # exact in double
    eps = float(np.float32(eps))
    s1, s2 = S1.double() * 2.0 ** -bits, S2.double() * 2.0 ** -bits
    beta = beta.double()
    mean, ex2 = s1 / M, s2 / M
    m2 = mean * mean
    var = (ex2 - m2).clamp(min=0)
    t = var + eps
    scale = t ** -0.5
    shift = beta - mean * scale
    g3, g7 = gamma(3), gamma(7)
    e_mean = g3 * mean.abs()
    e_raw = g3 * ex2.abs() + g7 * m2
    e_var = e_raw + U * ((ex2 - m2).abs() + e_raw)
    e_t = e_var + U * (t + e_var)
    assert bool((e_t < 0.25 * t).all()), "statistics too ill-conditioned for a meaningful bound"
    r_in = (t / (t - e_t)).sqrt() - 1
    r_scale = r_in + 2 * C_RSQRT * U * (1 + r_in)
    e_scale = scale * r_scale
    r_ms = (1 + g3) * (1 + r_scale) * (1 + U) - 1
    e_ms = (mean * scale).abs() * r_ms
    e_shift = e_ms + U * (shift.abs() + e_ms)
    return dict(scale=scale, shift=shift, mean=mean, var=var, e_scale=e_scale, e_shift=e_shift, e_mean=e_mean, e_var=e_var)


def bn_moving_ref(moving, batch, e_batch, momentum):
    """common.h bn_moving_update: a = fl(moving mom), w = fl(1 - mom), b = fl(batch w), a + b.  Returns (fp64 value, bound)."""
    mom = float(np.float32(momentum))
    moving, batch = moving.double(), batch.double()
    a, w = moving * mom, 1.0 - mom
    b = batch * w
    g2 = gamma(2)
    e_b = (batch.abs() * g2 + e_batch * (1 + g2)) * abs(w)
    e_a = U * a.abs()
    return a + b, e_a + e_b + U * (a.abs() + b.abs() + e_a + e_b)


def _rsqrt32(t32):
    """correctly rounded fp32 1/sqrt"""
    return (1.0 / np.sqrt(t32.astype(np.float64))).astype(np.float32)


def bn_affine_f32(S1, S2, M, eps, beta, bits=ACC_STAT_BITS):
    """fp32 NumPy restatement of bn_affine_from_sums (every line one rounding): scale, shift, mean, var as float32 arrays."""
    f = np.float32
    s1 = (S1.numpy().astype(np.float64) * 2.0 ** -bits).astype(f)
    s2 = (S2.numpy().astype(np.float64) * 2.0 ** -bits).astype(f)
    inv = f(1.0) / f(M)
    mean = s1 * inv
    ex2, m2 = s2 * inv, mean * mean
    var = np.maximum(ex2 - m2, f(0))
    t = var + f(eps)
    scale = _rsqrt32(t)
    ms = mean * scale
    return scale, beta.numpy().astype(f) - ms, mean, var, t


def bn_moving_f32(moving, batch, momentum):
    f = np.float32
    a, w = moving.astype(f) * f(momentum), f(1.0) - f(momentum)
    return a + batch.astype(f) * w


def bn_fwd_ref(y, sc, sf, relu):
    """z = round_lp(act(fma(y, scale, shift))) from the scale / shift the kernel saved.  Returns (ref, absref, k): the fma is one
    rounding; k = 2 over |y sc| + |sf| also admits an unfused multiply-add."""
    p = y.double() * sc.double()
    z = p + sf.double()
    return (z.clamp(min=0) if relu else z), p.abs() + sf.double().abs(), 2


def bn_zero_margin(y, sc, sf):
    """The ReLU mask zf > 0 is decided on fma(y, sc, sf), correctly rounded from the exact value: its sign is the exact sign
    unless the exact value is 0 or underflows.  Returns the number of such elements (fp64: the product is exact, the sum is
    rounded once, so the sign is exact here as well)."""
    z = y.double() * sc.double() + sf.double()
    return int((z.abs() < 2.0 ** -126).sum())


def bn_bwd_ref(dz, y, sc, sf, beta, A1, A2, M, relu, bits=ACC_GRAD_BITS):
    """bn_relu_bwd_apply_kernel in fp64: dy = sc (gg - k1 - (zf - beta) k2), k1 = S1/M, k2 = S2/M from the exact integer sums
    A1, A2 the kernel read.  Chain (k = 10): zf 2, zf - beta 1, k2 = fl(fl(S2) fl(1/M)) 3, product 1, k1 3 / gg - k1 1, the second
    subtraction 1, times sc 1 -- at most 10 roundings on any path, over absref = |sc| (|gg| + |k1| + (|y sc| + |sf| + |beta|) |k2|)."""
    sc, sf, beta = sc.double(), sf.double(), beta.double()
    p = y.double() * sc
    z = p + sf
    gg = dz.double() * (z > 0) if relu else dz.double()
    k1, k2 = A1.double() * 2.0 ** -bits / M, A2.double() * 2.0 ** -bits / M
    ref = sc * (gg - k1 - (z - beta) * k2)
    absref = sc.abs() * (gg.abs() + k1.abs() + (p.abs() + sf.abs() + beta.abs()) * k2.abs())
    return ref, absref, 10


def bn_sums_ref(dz, y, sc, sf, beta, relu):
    """bn_relu_bwd_reduce_kernel: column sums of gg and gg (zf - beta) in fp64, their absolute sums and the error the fp32 terms
    carry: gg is exact; gg (zf - beta) has zf (2 roundings), the subtraction, the product: gamma_4 |gg| (|y sc| + |sf| + |beta|)."""
    sc, sf, beta = sc.double(), sf.double(), beta.double()
    p = y.double() * sc
    z = p + sf
    gg = dz.double() * (z > 0) if relu else dz.double()
    t2 = gg * (z - beta)
    a2 = gg.abs() * (p.abs() + sf.abs() + beta.abs())
    return gg.sum(0), gg.abs().sum(0), t2.sum(0), a2.sum(0), gamma(4) * a2.sum(0)


def reduce_rows_per_block(M, C):
    """elementwise.hip reduce_rows_per_block"""
    chunks = min(max(32768 // max(C, 1), 8), 1024)
    return max(cdiv(M, chunks), 32)


def reduce_chain(M, C):
    """(longest fp32 chain of a column sum of the reduce kernels, number of fixed-point adds per column): a thread adds
    ceil(rows_per_block / 32) rows at most (TY >= 32), up to 8 LDS fold passes, then 32 partial sums."""
    rpb = reduce_rows_per_block(M, C)
    return cdiv(rpb, 32) + 8 + 32, cdiv(M, rpb)


def _fma32_t(a, b, c):
    return torch.from_numpy(fo._fma32(a.numpy(), b.numpy(), c.numpy()))


def bn_fwd_f32(y, sc32, sf32, relu, dt):
    zf = _fma32_t(y.float(), sc32, sf32)
    return (zf.clamp(min=0) if relu else zf).to(lp_torch(dt))


def bn_sums_f32(dz, y, sc32, sf32, beta, relu, M, C, skip_row=None, bits=ACC_GRAD_BITS):
    """fp32 restatement of the reduce kernel: per row chunk an fp32 column sum, rounded once to fixed point, integer total."""
    zf = _fma32_t(y.float(), sc32, sf32)
    gg = torch.where(zf > 0, dz.float(), torch.zeros(())) if relu else dz.float()
    t2 = gg * (zf - beta.float())
    if skip_row is not None:
        gg, t2 = gg.clone(), t2.clone()
        gg[skip_row] = 0
        t2[skip_row] = 0
    rpb = reduce_rows_per_block(M, C)
    A1, A2 = torch.zeros(C, dtype=torch.int64), torch.zeros(C, dtype=torch.int64)
    for r0 in range(0, M, rpb):
        A1 += (gg[r0:r0 + rpb].sum(0).double() * 2.0 ** bits).round().to(torch.int64)
        A2 += (t2[r0:r0 + rpb].sum(0).double() * 2.0 ** bits).round().to(torch.int64)
    return A1, A2


def bn_bwd_f32(dz, y, sc32, sf32, beta, A1, A2, M, relu, dt, bits=ACC_GRAD_BITS):
    f = np.float32
    zf = _fma32_t(y.float(), sc32, sf32)
    gg = torch.where(zf > 0, dz.float(), torch.zeros(())) if relu else dz.float()
    inv = f(1.0) / f(M)
    k1 = torch.from_numpy((A1.numpy().astype(np.float64) * 2.0 ** -bits).astype(f) * inv)
    k2 = torch.from_numpy((A2.numpy().astype(np.float64) * 2.0 ** -bits).astype(f) * inv)
    return (sc32 * (gg - k1 - (zf - beta.float()) * k2)).to(lp_torch(dt))


# ---------------------------------------------------------------------------------------------------------------------------
# residual backward
# ---------------------------------------------------------------------------------------------------------------------------
def residual_ref(dout, out, prev, scale, relu, accumulate):
    """Bit-exact dtrunk / dup (one rounding of an exactly representable fp32 expression each) and the fp64 dbias sums."""
    s32 = torch.tensor(scale, dtype=torch.float32)
    g = dout.float()
    if relu:
        g = torch.where(out.float() > 0, g, torch.zeros(()))
    up32 = s32 * g                                        # fp32(scale * g): one rounding
    dup = up32.to(dout.dtype)
    dtrunk = ((g + prev.float()) if accumulate else g).to(dout.dtype)
    t = g.double() * float(s32)
    return dtrunk, dup, t.sum(0), t.abs().sum(0)


# ---------------------------------------------------------------------------------------------------------------------------
# pools
# ---------------------------------------------------------------------------------------------------------------------------
def maxpool_ref(x):
    """x: [N,H,W,C] storage type (CPU).  First-maximum 3x3 / stride 2 / valid: (y in the storage type, argmax uint8), scan order
    ky, kx; numpy's argmax returns the first occurrence."""
    xf = x.float().numpy()
    N, H, W, C = xf.shape
    OH, OW = (H - 3) // 2 + 1, (W - 3) // 2 + 1
    win = np.stack([xf[:, ky:ky + 2 * OH - 1:2, kx:kx + 2 * OW - 1:2, :] for ky in range(3) for kx in range(3)], axis=3)   # [N,OH,OW,9,C]
    am = win.argmax(axis=3)
    y = np.take_along_axis(win, am[:, :, :, None, :], axis=3)[:, :, :, 0, :]
    return torch.from_numpy(y).to(x.dtype), torch.from_numpy(am.astype(np.uint8))


def maxpool_bwd_ref(dy, am, H, W):
    """fp64 gradient and the sum of |addends| from the argmax map: input (iy, ix) receives dy of every window whose first maximum
    sits there (<= 4 addends, from 0)."""
    d = dy.double().numpy()
    a = am.numpy()
    N, OH, OW, C = d.shape
    ref, absref = np.zeros((N, H, W, C)), np.zeros((N, H, W, C))
    for ky in range(3):
        for kx in range(3):
            m = (a == ky * 3 + kx)
            ref[:, ky:ky + 2 * OH - 1:2, kx:kx + 2 * OW - 1:2, :] += d * m
            absref[:, ky:ky + 2 * OH - 1:2, kx:kx + 2 * OW - 1:2, :] += np.abs(d) * m
    return torch.from_numpy(ref), torch.from_numpy(absref)


def avgpool3s1_ref(x):
    """TF 'SAME' 3x3 stride-1 average over the in-map taps, fp64: (ref, absref).  Kernel chain: <= 9 adds, fl(1 / taps), the
    product: k = 11."""
    xd = x.double()
    N, H, W, C = xd.shape

    def f(t):
        s = torch.zeros_like(t)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                ys, ye = max(0, -dy), min(H, H - dy)
                xs, xe = max(0, -dx), min(W, W - dx)
                s[:, ys:ye, xs:xe] += t[:, ys + dy:ye + dy, xs + dx:xe + dx]
        return s
    ty = torch.tensor([(i > 0) + 1 + (i + 1 < H) for i in range(H)], dtype=torch.float64).view(1, H, 1, 1)
    tx = torch.tensor([(i > 0) + 1 + (i + 1 < W) for i in range(W)], dtype=torch.float64).view(1, 1, W, 1)
    return f(xd) / (ty * tx), f(xd.abs()) / (ty * tx)


# ---------------------------------------------------------------------------------------------------------------------------
# embedding head
# ---------------------------------------------------------------------------------------------------------------------------
def head_bn_ref(y, beta, mm, mv, training, momentum, eps):
    """head_bn_fwd_kernel in fp64 with bounds.  Training: s = sum_n y (N adds), mean = s / N (gamma_{N+1}); d = y - mean,
    q = sum d^2 (each term: d carries e_mean + u|d|; square and add), var = q / N; rstd = rsqrtf(var + eps);
    out = fl(fl((y - mean) rstd) + beta)."""
    y, beta = y.double(), beta.double()
    N = y.shape[0]
    eps = float(np.float32(eps))
    if training:
        mean = y.mean(0)
        e_mean = gamma(N + 1) * y.abs().mean(0)
        d = y - mean
        e_d = e_mean + U * (d.abs() + e_mean)                               # per element
        var = (d * d).mean(0)
        # |d'^2 - d^2| <= 2|d| e_d + e_d^2, then N + 2 roundings (product, N adds, division) over the sum of the squares
        e_var = ((2 * d.abs() * e_d + e_d * e_d).mean(0)) * (1 + gamma(N + 2)) + gamma(N + 2) * var
    else:
        mean, var = mm.double(), mv.double()
        e_mean, e_var = torch.zeros_like(mean), torch.zeros_like(var)
    t = var + eps
    e_t = e_var + U * (t + e_var)
    assert bool((e_t < 0.25 * t).all())
    r_in = (t / (t - e_t)).sqrt() - 1
    r_rstd = r_in + 2 * C_RSQRT * U * (1 + r_in)
    rstd = t ** -0.5
    d = y - mean
    e_d = e_mean + U * (d.abs() + e_mean)
    prod = d * rstd
    e_prod = (d.abs() + e_d) * rstd * r_rstd + e_d * rstd + U * (prod.abs() + (d.abs() + e_d) * rstd * r_rstd + e_d * rstd)
    out = prod + beta
    e_out = e_prod + U * (out.abs() + e_prod) + U * prod.abs()      # the last u |prod|: a fused multiply-add rounds once, covered either way
    return dict(out=out, e_out=e_out, mean=mean, e_mean=e_mean, var=var, e_var=e_var, rstd=rstd, e_rstd=rstd * r_rstd)


def head_bn_f32(y, beta, mm, mv, training, eps):
    f = np.float32
    y, beta = y.numpy().astype(f), beta.numpy().astype(f)
    N = y.shape[0]
    if training:
        s = np.zeros(y.shape[1], f)
        for n in range(N):
            s = s + y[n]
        mean = s / f(N)
        q = np.zeros(y.shape[1], f)
        for n in range(N):
            d = y[n] - mean
            q = q + d * d
        var = q / f(N)
    else:
        mean, var = mm.numpy().astype(f), mv.numpy().astype(f)
    rstd = _rsqrt32(var + f(eps))
    return (y - mean) * rstd + beta, mean, var, rstd


def head_bn_bwd_ref(dout, y, mean, rstd, N):
    """head_bn_bwd_kernel in fp64 from the mean / rstd the forward saved (fp32 inputs of the formula).  s1: N adds; s2: N terms
    of 3 roundings + N adds; k1, k2: a division each; xh = (y - mean) rstd: 2; the result rstd (g - k1 - xh k2): 4 more.
    k = 2 N + 12 over the absolute sum bounds every path.  Returns (ref, absref, k, dbeta_ref, dbeta_abs)."""
    g, y, mean, rstd = dout.double(), y.double(), mean.double(), rstd.double()
    xh = (y - mean) * rstd
    axh = (y.abs() + mean.abs()) * rstd.abs()
    k1, k2 = g.mean(0), (g * xh).mean(0)
    a1, a2 = g.abs().mean(0), (g.abs() * axh).mean(0)
    ref = rstd * (g - k1 - xh * k2)
    absref = rstd.abs() * (g.abs() + a1 + axh * a2)
    return ref, absref, 2 * N + 12, g.sum(0), g.abs().sum(0)


def l2norm_ref(x, eps):
    """l2norm_fwd_kernel: per-lane chain of ceil(E / 64) fused or unfused multiply-adds, 6 butterfly adds, rsqrtf, one product.
    Returns (out, bound, s, e_s): s = sum x^2 and its fp32 error bound (the clamp s < eps is decided on the fp32 s)."""
    x = x.double()
    E = x.shape[1]
    eps = float(np.float32(eps))
    s = (x * x).sum(1, keepdim=True)
    e_s = gamma(2 * cdiv(E, 64) + 6) * s
    t = s.clamp(min=eps)
    r = t ** -0.5
    e_t = torch.where(s + e_s < eps, torch.zeros_like(s), e_s)           # clearly clamped rows: r = rsqrt(eps) whatever s is
    r_in = (t / (t - e_t)).sqrt() - 1
    r_r = r_in + 2 * C_RSQRT * U * (1 + r_in)
    out = x * r
    return out, out.abs() * (r_r + U * (1 + r_r)), s, e_s


def l2norm_f32(x, eps):
    f = np.float32
    x = x.numpy().astype(f)
    N, E = x.shape
    pad = np.zeros((N, cdiv(E, 64) * 64), f)
    pad[:, :E] = x
    lanes = pad.reshape(N, -1, 64)
    s = np.zeros((N, 64), f)
    for t in range(lanes.shape[1]):
        s = s + lanes[:, t] * lanes[:, t]
    s = fo._wave_sum32(s)
    r = _rsqrt32(np.maximum(s, f(eps)))
    return x * r[:, None], s


def l2norm_bwd_ref(x, dout, eps):
    """l2norm_bwd_kernel: clamped rows r dout; others r (dout - x r r d), d = <x, dout>.  Bound: d and s by their chains
    (gamma_{2 ceil(E/64) + 6}), r by the argument error and C_RSQRT ulps, then 5 roundings of the expression."""
    x, g = x.double(), dout.double()
    E = x.shape[1]
    eps = float(np.float32(eps))
    kc = 2 * cdiv(E, 64) + 6
    s = (x * x).sum(1, keepdim=True)
    d = (x * g).sum(1, keepdim=True)
    e_s, e_d = gamma(kc) * s, gamma(kc) * (x.abs() * g.abs()).sum(1, keepdim=True)
    clamped = s < eps
    t = s.clamp(min=eps)
    r = t ** -0.5
    e_t = torch.where(clamped, torch.zeros_like(s), e_s)
    r_in = (t / (t - e_t)).sqrt() - 1
    r_r = r_in + 2 * C_RSQRT * U * (1 + r_in)
    ref = torch.where(clamped, r * g, r * (g - x * r * r * d))
    # first order in the relative errors: r enters three times in the second term, once in the first; 5 roundings on top
    q = x.abs() * r * r * r
    bound = torch.where(clamped, (r * g).abs() * (r_r + 2 * U),
                        (r * g).abs() * (r_r + gamma(3)) * (1 + r_r) + q * (d.abs() * ((1 + r_r) ** 3 - 1 + gamma(6)) + e_d * (1 + r_r) ** 3 * (1 + gamma(6))))
    margin_ok = bool((((s - eps).abs() > e_s) | (s == 0)).all())           # the clamp decision is unambiguous in fp32
    return ref, bound, margin_ok


def l2norm_inputs(N, E, seed, eps=1e-10):
    """fp32 rows with, when N >= 4: row 0 all zero, row 1 with sum x^2 = eps / 100, row 2 with 100 eps (both sides of the clamp)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, E, generator=g) * 3.0 + 1.5
    if N >= 4:
        x[0] = 0
        for row, target in ((1, eps / 100), (2, eps * 100)):
            v = torch.randn(E, generator=g).double()
            x[row] = (v * math.sqrt(target) / v.norm()).float()
    return x, torch.randn(N, E, generator=g)


# ---------------------------------------------------------------------------------------------------------------------------
# softmax cross-entropy
# ---------------------------------------------------------------------------------------------------------------------------
def softmax_inputs(N, C, ld, seed):
    """logits fp32 [N, ld] at scale 3 with a per-row offset of +-80 (the max subtraction), padding columns poisoned with 1e30 (the
    kernel must not read them), labels covering column 0 and C - 1."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, ld, generator=g) * 3.0
    off = torch.tensor([80.0 if i % 2 else -80.0 for i in range(N)]).view(N, 1)
    x = x + off
    x[:, C:] = 1e30
    labels = torch.randint(0, C, (N,), generator=g, dtype=torch.int32)
    labels[0], labels[1 % N] = 0, C - 1
    if N > 2:
        labels[2] = labels[N - 1]          # a repeated class
    return x, labels


def softmax_ref(x, labels, C, grad_scale):
    """softmax_xent_kernel in fp64.  Per row: mx exact; e_c = __expf(x_c - mx): the subtraction rounds (rel u of |x_c - mx| in
    the argument -> |x_c - mx| u relative in e_c), then C_EXP + 1.45 |x_c - mx| ulps; s: per thread ceil(C / 256) adds, 6 butterfly
    adds, 3 adds over the waves.  loss row = fl(fl(fl(logf(s)) + mx) - x_lab) / N; dlogits = (e_c fl(1 / s) - onehot) grad_scale.
    Returns dict with loss, e_loss, g (fp64 [N, C]), e_g (fp32 error of g before the storage rounding), dbias, e_dbias."""
    N = x.shape[0]
    xs = x[:, :C].double()
    mx = xs.max(1, keepdim=True).values
    a = xs - mx                                           # <= 0
    e = a.exp()
    r_e = U * a.abs() + U * a.abs() * U + 2 * U * (C_EXP + EXP_ARG_ULPS * (a.abs() * (1 + U)))      # relative error of every e_c
    ks = cdiv(C, 256) + 6 + 3
    s = e.sum(1, keepdim=True)
    e_s = (e * r_e).sum(1, keepdim=True) * (1 + gamma(ks)) + gamma(ks) * s
    r_s = e_s / s
    lab = labels.long().view(N, 1)
    xl = xs.gather(1, lab)
    lse = s.log()
    row = lse + mx - xl
    # logf: argument error r_s / (1 - r_s) absolute in the log, C_LOG ulps of the result; two more adds; the division by N; the
    # conversion to fixed point (2^-41 per row)
    e_log = r_s / (1 - r_s) + 2 * C_LOG * U * lse.abs()
    e_row = e_log + U * ((lse + mx).abs() + e_log) + U * (row.abs() + e_log + U * (lse + mx).abs())
    loss = row.sum() / N
    e_rows = (e_row / N + U * (row.abs() + e_row) / N + 2.0 ** -41).sum()
    e_loss = e_rows + U * (loss.abs() + e_rows)           # acc_get rounds the total to fp32
    onehot = torch.zeros_like(xs).scatter_(1, lab, 1.0)
    gs = float(np.float32(grad_scale))
    p = e / s
    r_p = (1 + r_e) * (1 + r_s / (1 - r_s)) * (1 + gamma(2)) - 1          # e_c, 1 / s (its own rounding), the product
    g = (p - onehot) * gs
    e_g = (p * r_p + U * ((p - onehot).abs() + p * r_p)) * abs(gs) + U * (g.abs() + p * r_p * abs(gs))
    dbias = g.sum(0)
    e_dbias = e_g.sum(0) + N * 2.0 ** -41                  # every row adds its fp32 g, rounded once to 2^-40
    return dict(loss=loss, e_loss=e_loss, g=g, e_g=e_g, dbias=dbias, e_dbias=e_dbias, s=s, lse=lse)


def softmax_f32(x, labels, C, grad_scale, dt, skip_col=None):
    """fp32 restatement in the kernel's order (256 threads striding the columns, wave butterflies, 4 wave totals)."""
    f = np.float32
    N = x.shape[0]
    xs = x[:, :C].numpy().astype(f)
    mx = xs.max(1, keepdims=True)
    a = xs - mx
    e = np.exp(a.astype(np.float64)).astype(f)            # correctly rounded fp32 exp
    if skip_col is not None:
        e = e.copy()
        e[:, skip_col] = 0
    pad = np.zeros((N, cdiv(C, 256) * 256), f)
    pad[:, :C] = e
    th = pad.reshape(N, -1, 256)
    acc = np.zeros((N, 256), f)
    for t in range(th.shape[1]):
        acc = acc + th[:, t]
    w = fo._wave_sum32(acc.reshape(N, 4, 64))
    s = ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]
    lab = labels.long().numpy()
    lse = np.log(s.astype(np.float64)).astype(f)
    rows = ((lse + mx[:, 0]) - xs[np.arange(N), lab]) / f(N)
    acc_i = np.rint(rows.astype(np.float64) * 2.0 ** ACC_GRAD_BITS).astype(np.int64).sum()
    loss = f(float(acc_i) * 2.0 ** -ACC_GRAD_BITS)
    inv = f(1.0) / s
    onehot = np.zeros_like(xs)
    onehot[np.arange(N), lab] = 1
    g = (np.exp(a.astype(np.float64)).astype(f) * inv[:, None] - onehot) * f(grad_scale)
    dbias = np.rint(g.astype(np.float64) * 2.0 ** ACC_GRAD_BITS).astype(np.int64).sum(0)
    return loss, torch.from_numpy(g).to(lp_torch(dt)), torch.from_numpy(dbias), dict(a=a, e=e, s=s, lse=lse)


# ---------------------------------------------------------------------------------------------------------------------------
# triplet loss
# ---------------------------------------------------------------------------------------------------------------------------
def triplet_inputs(T, E, alpha, seed):
    """fp32 [3T, E] rows (a, p, n): a mix of clearly active and clearly inactive triplets; the last triplet has p == n bit for bit,
    which with alpha = 0 is an exactly zero hinge (pos and neg are the same fp32 sums).  Every other hinge value is moved away
    from 0 by more than the fp32 error of pos - neg + alpha."""
    g = torch.Generator().manual_seed(seed)
    emb = torch.randn(3 * T, E, generator=g)
    emb = emb / emb.norm(dim=1, keepdim=True)
    for t in range(T):
        a = emb[3 * t]
        if t % 2 == 0:          # active: the negative is close to the anchor
            emb[3 * t + 2] = a + 0.05 * emb[3 * t + 2]
        else:                   # inactive: the positive is close to the anchor, the negative far
            emb[3 * t + 1] = a + 0.05 * emb[3 * t + 1]
    emb[3 * (T - 1) + 2] = emb[3 * (T - 1) + 1]
    return emb.contiguous()


def triplet_ref(emb, T, E, alpha):
    """triplet_loss_kernel in fp64.  pos, neg: per lane ceil(E / 64) terms (difference, square, add: 3 roundings each) and 6
    butterfly adds: gamma_{3 ceil(E/64) + 6} each; l = fl(fl(pos - neg) + alpha).  Returns loss, e_loss, grad, e_grad, l, e_l."""
    al = float(np.float32(alpha))
    e = emb.double().view(T, 3, E)
    a, p, n = e[:, 0], e[:, 1], e[:, 2]
    pos, neg = ((a - p) ** 2).sum(1), ((a - n) ** 2).sum(1)
    k = 3 * cdiv(E, 64) + 6
    e_pn = gamma(k) * (pos + neg)
    l = pos - neg + al
    e_l = e_pn + U * ((pos - neg).abs() + e_pn) + U * (l.abs() + e_pn)
    on = (l > 0).double()
    rows = l.clamp(min=0) / T
    e_rows = on * (e_l / T + U * rows) + 2.0 ** -41
    loss = rows.sum()
    e_loss = e_rows.sum() + U * (loss + e_rows.sum())
    s = 2.0 * on / T                                       # fl(fl(2 on) / T): one rounding; the difference: one; the product: one
    grad = torch.stack([s[:, None] * (n - p), s[:, None] * (p - a), s[:, None] * (a - n)], 1).reshape(3 * T, E)
    e_grad = gamma(3) * grad.abs()
    return dict(loss=loss, e_loss=e_loss, grad=grad, e_grad=e_grad, l=l, e_l=e_l, same=(e[:, 1] == e[:, 2]).all(1))


def triplet_f32(emb, T, E, alpha):
    f = np.float32
    e = emb.numpy().astype(f).reshape(T, 3, E)
    a, p, n = e[:, 0], e[:, 1], e[:, 2]

    def sq(u, v):
        d = np.zeros((T, cdiv(E, 64) * 64), f)
        d[:, :E] = u - v
        lanes = d.reshape(T, -1, 64)
        acc = np.zeros((T, 64), f)
        for t in range(lanes.shape[1]):
            acc = acc + lanes[:, t] * lanes[:, t]
        return fo._wave_sum32(acc)
    pos, neg = sq(a, p), sq(a, n)
    l = pos - neg + f(alpha)
    rows = np.maximum(l, f(0)) / f(T)
    loss = f(float(np.rint(rows.astype(np.float64) * 2.0 ** ACC_GRAD_BITS).astype(np.int64).sum()) * 2.0 ** -ACC_GRAD_BITS)
    s = (f(2) * (l > 0).astype(f) / f(T))[:, None]
    grad = np.stack([s * (n - p), s * (p - a), s * (a - n)], 1).reshape(3 * T, E)
    return loss, grad, l


# ---------------------------------------------------------------------------------------------------------------------------
# image ops
# ---------------------------------------------------------------------------------------------------------------------------
def resize_ref(img, OH, OW):
    """resize_bilinear_kernel in fp64: half-pixel centres, src = (dst + 0.5) in/out - 0.5, lower = max(floor, 0), upper =
    min(ceil, in - 1), weight = src - floor(src).  The kernel computes sy = fl(H / OH), fy = fl(fl((oy + 0.5) sy) - 0.5): 3
    roundings of a value <= H, so |fy - exact| <= gamma_3 (H + 0.5) =: e_pos (0 for the identity, where every step is exact).  The
    interpolant is continuous and piecewise linear in the position, so the position error moves the result by at most e_pos times
    the steepest slope |v1 - v0| among the cells within e_pos of the exact position: where that position is (nearly) an integer
    (96 -> 160 has such columns) the fp32 position may fall in the neighbouring cell, and that cell's slope is taken into
    account, nothing is excluded.  On top: fl(f - floor f) rounds once, the three lerps round 3 times each over <= 3 max|v|.
    Returns (ref, bound) [N,OH,OW,3]."""
    x = img.double()
    N, H, W, _ = x.shape

    def axis(n_in, n_out):
        o = torch.arange(n_out, dtype=torch.float64)
        f = (o + 0.5) * (n_in / n_out) - 0.5
        e_pos = gamma(3) * (n_in + 0.5) if n_in != n_out else 0.0
        cells = []
        for ff in (f, f - e_pos, f + e_pos):
            cells.append((ff.floor().clamp(min=0, max=n_in - 1).long(), ff.ceil().clamp(min=0, max=n_in - 1).long()))
        return cells, f - f.floor(), e_pos
    ycells, ly, ey = axis(H, OH)
    xcells, lx, ex = axis(W, OW)
    ly, lx = ly.view(1, OH, 1, 1), lx.view(1, 1, OW, 1)

    def lerp_x(rows, xc):
        a, b = x[:, rows][:, :, xc[0]], x[:, rows][:, :, xc[1]]
        return a + (b - a) * lx, (b - a).abs()
    (y0, y1), (x0, x1) = ycells[0], xcells[0]
    top, _ = lerp_x(y0, xcells[0])
    bot, _ = lerp_x(y1, xcells[0])
    ref = top + (bot - top) * ly
    slope_x = torch.zeros_like(ref)
    slope_y = torch.zeros_like(ref)
    for xc in xcells:
        for rows in (y0, y1):
            slope_x = torch.maximum(slope_x, lerp_x(rows, xc)[1])
    for yc in ycells:
        slope_y = torch.maximum(slope_y, (lerp_x(yc[1], xcells[0])[0] - lerp_x(yc[0], xcells[0])[0]).abs())
    mag = torch.stack([x[:, r][:, :, c].abs() for r in (y0, y1) for c in (x0, x1)]).amax(0)
    bound = slope_x * (ex + U) + slope_y * (ey + U) + gamma(9) * 3 * mag
    return ref, bound


def normalize_ref(img, mode):
    """img_stats / img_apply kernels in fp64 for [N,HW,3] input (u8 or fp32 values).  mode 0: (2x - (min + max)) / max(max - min,
    1e-3): sub and den round once each, 2x exact, the difference and the division round: k = 4 over (2|x| + |sub|) / den, and den's
    own relative error u enters through the quotient (in k).  mode 1: (x - mean) / max(std, 1/sqrt(n)); the sums are fixed point
    (2^-20 per contribution of <= 8 x 4 waves), each wave's fp32 partial carries its chain error: mean and var get explicit
    bounds, var's cancellation included.  Returns (ref, bound_before_storage_rounding) [N,HW,3]."""
    x = img.double()
    N, HW, _ = x.shape
    n = HW * 3
    if mode == 0:
        mx, mn = x.amax((1, 2), keepdim=True), x.amin((1, 2), keepdim=True)
        sub, den = mn + mx, (mx - mn).clamp(min=float(np.float32(1e-3)))
        ref = (2 * x - sub) / den
        return ref, gamma(4) * (2 * x.abs() + sub.abs()) / den
    # per wave: a lane adds <= ceil(n / (16 * 2048)) * 16 + 2 values (vector trips of 16 u8 / 4 fp32, head and tail), 6 butterfly adds
    chain = cdiv(n, 2048) + 16 + 6
    s1, s2 = x.sum((1, 2), keepdim=True), (x * x).sum((1, 2), keepdim=True)
    a1 = x.abs().sum((1, 2), keepdim=True)
    e_s1 = gamma(chain) * a1 + 32 * 2.0 ** -20
    e_s2 = gamma(2 * chain) * s2 + 32 * 2.0 ** -20             # a product and an add per value
    mean, ex2 = s1 / n, s2 / n
    e_mean = (e_s1 / n) * (1 + gamma(3)) + gamma(3) * mean.abs()          # acc_get, (float) count, the division
    e_ex2 = (e_s2 / n) * (1 + gamma(3)) + gamma(3) * ex2
    m2 = mean * mean
    e_m2 = 2 * mean.abs() * e_mean + e_mean ** 2 + U * (m2 + 2 * mean.abs() * e_mean + e_mean ** 2)
    var = (ex2 - m2).clamp(min=0)
    e_var = e_ex2 + e_m2 + U * (var + e_ex2 + e_m2)
    floor = float(n) ** -0.5
    std = var.sqrt()
    # sqrt of a perturbed argument: |sqrt(v + e) - sqrt(v)| <= sqrt(e) always, <= e / (2 sqrt(v)) when v > e
    e_std = torch.where(var > 4 * e_var, e_var / (2 * (var - e_var).clamp(min=1e-300).sqrt()), e_var.sqrt()) + U * std
    den = std.clamp(min=floor)
    e_den = torch.maximum(e_std, torch.full_like(std, 2 * C_RSQRT * U * floor)) + U * den
    assert bool((e_den < 0.25 * den).all())
    ref = (x - mean) / den
    num_e = e_mean + U * ((x - mean).abs() + e_mean)
    bound = num_e / (den - e_den) + (x - mean).abs() * e_den / (den * (den - e_den)) + U * (ref.abs() + num_e / (den - e_den))
    return ref, bound
