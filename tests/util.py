"""Shared helpers for the GPU parity tests (everything goes through the C ABI)."""
import ctypes as C

import numpy as np
import torch

from facenet_amd import _lib
from facenet_amd._lib import ConvDesc


# fixed-point accumulators of the C ABI (fn_acc_t, include/facenet_hip.h): value = integer * 2^-bits
ACC_STAT_BITS, ACC_GRAD_BITS = 20, 40


def to_acc(t, bits):
    """fp tensor -> int64 fixed-point accumulator contents (what a kernel's contributions would have summed to)."""
    return (t.double() * float(2 ** bits)).round().to(torch.int64)


def from_acc(t, bits):
    return (t.double() / float(2 ** bits)).float()


def stream():
    return torch.cuda.current_stream().cuda_stream


def ptr(t, off=0):
    return t.data_ptr() + off * t.element_size()


def lp_dtype(code):
    return torch.bfloat16 if code == _lib.FN_BF16 else torch.float16


def conv_desc(N, H, W, Cin, Cout, kh, kw, stride, ph, pw, dt, ld_x=None, ld_y=None):
    d = ConvDesc()
    d.N, d.H, d.W, d.Cin = N, H, W, Cin
    d.OH, d.OW, d.Cout = (H + 2 * ph - kh) // stride + 1, (W + 2 * pw - kw) // stride + 1, Cout
    d.KH, d.KW, d.stride, d.pad_h, d.pad_w = kh, kw, stride, ph, pw
    d.dtype = dt
    d.ld_x = ld_x or Cin
    d.ld_y = ld_y or Cout
    d.scale = 1.0
    return d


def ref_conv(x_nhwc, w_ohwi, stride, ph, pw):
    """fp32 reference on the CPU from the SAME low-precision-rounded operands."""
    x = x_nhwc.float().cpu().permute(0, 3, 1, 2)
    w = w_ohwi.float().cpu().permute(0, 3, 1, 2)
    return torch.nn.functional.conv2d(x, w, None, stride=stride, padding=(ph, pw)).permute(0, 2, 3, 1).contiguous()


def rel_err(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


from tests.util_data import structured_images  # noqa: E402,F401


# ---- element-wise error bounds ---------------------------------------------------------------------------------------------
# A kernel output is an fp32 accumulation of K products of low-precision operands (exact in fp32), rounded once to the storage
# type.  Whatever the summation order, the fp32 sum s of terms t_i obeys |s - sum t_i| <= gamma_K * sum |t_i| (Higham, Accuracy
# and Stability of Numerical Algorithms, 2nd ed., eq. 3.5), and the rounding adds at most u_lp * |s|.  The bound below holds for
# every element, so a single wrong element -- a ragged tail, a border pixel, one member of a grouped launch -- fails it, where a
# relative error over the whole tensor would average it away.
U_FP32 = 2.0 ** -24
U_LP = {_lib.FN_BF16: 2.0 ** -8, _lib.FN_F16: 2.0 ** -11}
ETA_LP = {_lib.FN_BF16: 0.0, _lib.FN_F16: 2.0 ** -25}      # half the spacing of the f16 subnormals (bf16 has fp32's exponent range)


def gamma(k):
    """gamma_K = K u / (1 - K u) for fp32 (u = 2^-24): the worst-case relative error of a K-term fp32 sum in any order."""
    ku = float(k) * U_FP32
    assert ku < 0.5, k
    return ku / (1.0 - ku)


def bitpattern(shape, dt, device="cuda"):
    """A fixed, recognisable bit pattern for bytes a kernel must leave alone (compare with `same_bits`)."""
    n = int(np.prod(shape))
    bits = ((torch.arange(n, dtype=torch.int32) * 40503 + 0x3A5C) & 0x3FFF).to(torch.int16)     # finite values of either type
    return bits.view(lp_dtype(dt)).reshape(shape).to(device)


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int16).cpu(), b.contiguous().view(torch.int16).cpu()) if a.element_size() == 2 \
        else torch.equal(a.cpu(), b.cpu())


def assert_elementwise(got, ref, absref, k, dt, what="", out_f32=False):
    """|got - ref| <= u_lp (|ref| + gamma_K absref) + gamma_K absref (+ half an f16 subnormal step) at EVERY element.
    ref: the exact result in fp64 from the same rounded operands; absref: the same sum over absolute values; k: the number of
    fp32 operations in the longest chain (the GEMM depth plus what the epilogue adds).  NaN in `got` fails.  out_f32: the result
    is stored in fp32 (no low-precision rounding)."""
    got, ref, absref = got.double().cpu(), ref.double().cpu(), absref.double().cpu()
    assert got.shape == ref.shape == absref.shape, (what, got.shape, ref.shape, absref.shape)
    g = gamma(k)
    u, eta = (U_FP32, 0.0) if out_f32 else (U_LP[dt], ETA_LP[dt])
    bound = u * (ref.abs() + g * absref) + g * absref + eta
    err = (got - ref).abs()
    bad = ~(err <= bound)
    if bool(bad.any()):
        excess = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err - bound)
        i = int(excess.reshape(-1).argmax())
        idx = tuple(int(v) for v in np.unravel_index(i, tuple(got.shape)))
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements outside the bound; worst at {idx}: got "
                             f"{float(got[idx]):.8g}, fp64 {float(ref[idx]):.8g}, |err| {float(err[idx]):.3g} > bound {float(bound[idx]):.3g}")


def assert_acc_sums(acc, ref, absref, bits, n_tiles, what="", term_err=None, rows=128):
    """Fixed-point accumulators (fn_acc_t: `stats`, `bn_acc`, `rb_dbias`): every workgroup adds the fp32 sum of its <= `rows`
    terms per column, rounded once to 2^-bits.  acc: int64 sums (replicas already added); ref / absref: fp64 column sums of the
    exact terms and of their absolute values; term_err: fp64 column sums of the error each fp32 term already carries (None: the
    terms are exact).  Bound: term_err + gamma_rows (absref + term_err) + n_tiles 2^-bits."""
    got = acc.double().cpu() * 2.0 ** -bits
    ref, absref = ref.double().cpu(), absref.double().cpu()
    te = torch.zeros_like(ref) if term_err is None else term_err.double().cpu()
    bound = te + gamma(rows) * (absref + te) + n_tiles * 2.0 ** -bits
    err = (got - ref).abs()
    bad = ~(err <= bound)
    if bool(bad.any()):
        i = int((err - bound).reshape(-1).argmax())
        idx = tuple(int(v) for v in np.unravel_index(i, tuple(got.shape)))
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} sums outside the bound; worst at {idx}: got {float(got[idx]):.10g}, "
                             f"fp64 {float(ref[idx]):.10g}, |err| {float(err[idx]):.3g} > bound {float(bound[idx]):.3g}")


def conv_fp64(x_nhwc, w_ohwi, stride, ph, pw):
    """(fp64 forward convolution, the same over |x| |w|) on the CPU from the rounded operands, NHWC."""
    x = x_nhwc.double().cpu().permute(0, 3, 1, 2)
    w = w_ohwi.double().cpu().permute(0, 3, 1, 2)
    f = lambda a, b: torch.nn.functional.conv2d(a, b, None, stride=stride, padding=(ph, pw)).permute(0, 2, 3, 1).contiguous()
    return f(x, w), f(x.abs(), w.abs())


def dgrad_fp64(dy_nhwc, w_ohwi, H, W, stride, ph, pw):
    """(fp64 data gradient of the forward convolution, the same over |dy| |w|) on the CPU, NHWC [N,H,W,Cin]."""
    w = w_ohwi.double().cpu().permute(0, 3, 1, 2)
    N = dy_nhwc.shape[0]

    def f(dy, ww):
        x = torch.zeros(N, ww.shape[1], H, W, dtype=torch.float64, requires_grad=True)
        y = torch.nn.functional.conv2d(x, ww, None, stride=stride, padding=(ph, pw))
        y.backward(dy.double().cpu().permute(0, 3, 1, 2))
        return x.grad.permute(0, 2, 3, 1).contiguous()
    return f(dy_nhwc, w), f(dy_nhwc.abs(), w.abs())


# ---- weight gradients -------------------------------------------------------------------------------------------------------
# dW[co][ky][kx][ci] = sum over the M = N*OH*OW output pixels of dY[n,oy,ox,co] * X[n, oy*s - ph + ky, ox*s - pw + kx, ci]: an fp32
# sum of M exact products, stored in fp32 (assert_elementwise(..., out_f32=True)).  A launch split over pixels adds `splits`
# partial sums (global atomics into dW, or slabs added by the ordered reduce), in any order: k = M + splits + 2.
# The bound is about M 2^-24 absref, one missing pixel term about absref / M: the check sees a single dropped term only while
# M^2 << 2^24, so every weight-gradient case keeps M <= 2048 (M^2 2^-24 <= 1/4).
WGRAD_MAX_M = 2048


def lp_randn(shape, dt, scale=1.0, seed=0):
    """Seeded normal values rounded to the storage type, on the CPU."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(lp_dtype(dt))


def wgrad_pixels(case):
    """M = N*OH*OW of a (N, H, W, Cin, Cout, kh, kw, stride, ph, pw) case: the number of terms of one dW element."""
    N, H, W, Cin, Cout, kh, kw, s, ph, pw = case[:10]
    return N * ((H + 2 * ph - kh) // s + 1) * ((W + 2 * pw - kw) // s + 1)


def wgrad_k(M, splits):
    """Length of the longest fp32 chain behind one dW element: M products, `splits` partial sums, the store."""
    return M + max(int(splits), 1) + 2


def wgrad_operands(case, dt, seed):
    """(x [N,H,W,Cin], dy [N,OH,OW,Cout]) of a weight-gradient case: rounded operands on the CPU, shared by the GPU tests and
    the host test of their bound."""
    N, H, W, Cin, Cout, kh, kw, s, ph, pw = case[:10]
    OH, OW = (H + 2 * ph - kh) // s + 1, (W + 2 * pw - kw) // s + 1
    return lp_randn((N, H, W, Cin), dt, seed=seed), lp_randn((N, OH, OW, Cout), dt, seed=seed + 1)


def wgrad_fp64(x_nhwc, dy_nhwc, kh, kw, stride, ph, pw):
    """(fp64 weight gradient [Cout, kh, kw, Cin] of the convolution, the same sum over |x| |dy|) on the CPU from the rounded
    operands: tap (ky, kx) is the product of dY [M, Cout]^T with the strided window of the zero-padded x that tap reads."""
    x, dy = x_nhwc.double().cpu(), dy_nhwc.double().cpu()
    N, H, W, Cin = x.shape
    _, OH, OW, Cout = dy.shape
    assert OH == (H + 2 * ph - kh) // stride + 1 and OW == (W + 2 * pw - kw) // stride + 1, (x.shape, dy.shape)
    xp = torch.zeros(N, H + 2 * ph, W + 2 * pw, Cin, dtype=torch.float64)
    xp[:, ph:ph + H, pw:pw + W] = x
    g = dy.reshape(-1, Cout)

    def f(a, b):
        out = torch.empty(Cout, kh, kw, Cin, dtype=torch.float64)
        for ky in range(kh):
            for kx in range(kw):
                win = a[:, ky:ky + (OH - 1) * stride + 1:stride, kx:kx + (OW - 1) * stride + 1:stride]
                out[:, ky, kx] = b.t() @ win.reshape(-1, Cin)
        return out
    return f(xp, g), f(xp.abs(), g.abs())
