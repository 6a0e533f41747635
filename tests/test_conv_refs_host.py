"""The weight-gradient reference and bound of the GPU tests checked against each other, without a GPU: tests.util.wgrad_fp64
against a plain loop nest, then, for the geometry and storage type of every case of tests/test_gpu_conv_wgrad.py, the fp32 CPU
autograd gradient must stay inside the bound the GPU test applies, and three planted errors must fall outside it -- (a) one
element that misses one pixel's product, (b) one element taken from the neighbouring tap, (c) one element left at 0.  A kernel
that is wrong in one tap, one pixel or one channel therefore fails the GPU tests."""
import numpy as np
import pytest
import torch

from facenet_amd import _lib
from tests.test_gpu_conv_wgrad import ALL_WGRAD_CASES, NORM_CASES, REDUCE_CASES
from tests.util import WGRAD_MAX_M, assert_elementwise, wgrad_fp64, wgrad_k, wgrad_operands, wgrad_pixels

CASES = sorted(set(ALL_WGRAD_CASES))
NORM_GEOS = {g for g, _ in NORM_CASES}
FORCED = {g: s for g, s in REDUCE_CASES}


def _loops(x, dy, kh, kw, s, ph, pw):
    """dW[co][ky][kx][ci] = sum_{n,oy,ox} dY[n,oy,ox,co] X[n, oy s - ph + ky, ox s - pw + kx, ci], term by term in NumPy fp64."""
    x, dy = x.double().numpy(), dy.double().numpy()
    N, H, W, Cin = x.shape
    _, OH, OW, Cout = dy.shape
    dw, adw = np.zeros((Cout, kh, kw, Cin)), np.zeros((Cout, kh, kw, Cin))
    for n in range(N):
        for oy in range(OH):
            for ox in range(OW):
                for ky in range(kh):
                    for kx in range(kw):
                        iy, ix = oy * s - ph + ky, ox * s - pw + kx
                        if 0 <= iy < H and 0 <= ix < W:
                            dw[:, ky, kx, :] += np.outer(dy[n, oy, ox], x[n, iy, ix])
                            adw[:, ky, kx, :] += np.outer(np.abs(dy[n, oy, ox]), np.abs(x[n, iy, ix]))
    return dw, adw


@pytest.mark.parametrize("case", [(2, 7, 9, 8, 16, 3, 3, 2, 0, 0), (2, 3, 5, 8, 8, 1, 7, 1, 0, 3)], ids=["3x3 stride 2 valid", "1x7 same"])
def test_wgrad_fp64_equals_a_plain_loop_nest(case):
    for dt in (_lib.FN_BF16, _lib.FN_F16):
        x, dy = wgrad_operands(case, dt, 5)
        ref, aref = wgrad_fp64(x, dy, *case[5:])
        lr, la = _loops(x, dy, *case[5:])
        assert ref.shape == (case[4], case[5], case[6], case[3]) and float(ref.abs().max()) > 0
        tol = 1e-13 * la                                                   # two fp64 summation orders of the same exact terms
        assert bool((np.abs(ref.numpy() - lr) <= tol).all()) and bool((np.abs(aref.numpy() - la) <= tol).all())


def _terms(x, dy, case, idx):
    """The fp64 products behind element idx = (co, ky, kx, ci) of dW, one per output pixel (0 where the tap reads padding)."""
    N, H, W, Cin, Cout, kh, kw, s, ph, pw = case
    co, ky, kx, ci = idx
    OH, OW = dy.shape[1:3]
    xp = torch.zeros(N, H + 2 * ph, W + 2 * pw, dtype=torch.float64)
    xp[:, ph:ph + H, pw:pw + W] = x[..., ci].double()
    win = xp[:, ky:ky + (OH - 1) * s + 1:s, kx:kx + (OW - 1) * s + 1:s]
    return (win * dy[..., co].double()).reshape(-1)


@pytest.mark.parametrize("dt", [_lib.FN_BF16, _lib.FN_F16], ids=["bf16", "f16"])
@pytest.mark.parametrize("case", CASES, ids=["x".join(map(str, c)) for c in CASES])
def test_wgrad_bound_accepts_fp32_autograd_and_rejects_planted_errors(case, dt):
    N, H, W, Cin, Cout, kh, kw, s, ph, pw = case
    M = wgrad_pixels(case)
    assert M <= WGRAD_MAX_M
    x, dy = wgrad_operands(case, dt, 700)
    if case in NORM_GEOS:                      # the normalise-on-load cases read a ReLU output: half of the terms are zero
        x = torch.relu(x)
    ref, aref = wgrad_fp64(x, dy, kh, kw, s, ph, pw)
    wr = torch.zeros(Cout, Cin, kh, kw, requires_grad=True)
    yr = torch.nn.functional.conv2d(x.float().permute(0, 3, 1, 2), wr, None, stride=s, padding=(ph, pw))
    yr.backward(dy.float().permute(0, 3, 1, 2))
    got = wr.grad.permute(0, 2, 3, 1).contiguous()
    assert_elementwise(got, ref, aref, wgrad_k(M, 1), dt, f"{case} fp32 autograd", out_f32=True)     # the tightest k any GPU run uses
    # the widest k any GPU run of this case uses: a forced split, or one partial sum per 64-pixel stage / per pixel tile (<= M)
    k = wgrad_k(M, max(FORCED.get(case, 0), M))

    def rejected(bad, what):
        try:
            assert_elementwise(bad, ref, aref, k, dt, what, out_f32=True)
        except AssertionError:
            return True
        return False
    # the element: last output channel (ragged cout tile), last tap, the input channel of the ragged tail with the largest |dW|
    ci = int(ref[Cout - 1, kh - 1, kw - 1].abs().argmax())
    idx = (Cout - 1, kh - 1, kw - 1, ci)
    # (a) one pixel's product missing: a fixed pixel first; where that term happens to be tiny, the element's largest term
    t = _terms(x, dy, case, idx)
    assert abs(float(t.sum()) - float(ref[idx])) <= 1e-12 * float(aref[idx])
    bad = got.clone()
    bad[idx] = float(got[idx].double() - t[M // 2])
    if not rejected(bad, "(a) fixed pixel"):
        bad[idx] = float(got[idx].double() - t[int(t.abs().argmax())])
        assert rejected(bad, "(a) largest term"), (case, float(t.abs().max()), float(aref[idx]))
    # (b) the neighbouring tap's value (for a 1x1 layer, which has one tap: the neighbouring input channel, the next K column)
    bad = got.clone()
    if kh * kw > 1:
        nb = (Cout - 1, kh - 1, kw - 2, ci) if kw > 1 else (Cout - 1, kh - 2, kw - 1, ci)
    else:
        nb = (Cout - 1, 0, 0, ci - 1 if ci else 1)
    bad[idx] = got[nb]
    assert rejected(bad, "(b) neighbouring tap")
    # (c) left at zero
    bad = got.clone()
    bad[idx] = 0
    assert rejected(bad, "(c) zero")
