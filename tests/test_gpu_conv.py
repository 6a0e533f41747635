"""Implicit-GEMM convolution kernels (fwd / dgrad / wgrad) against an fp32 CPU convolution on the same
rounded operands.  Shapes cover every kernel size / stride / padding of Inception-ResNet-v1, ragged M,
odd channel counts (80, 10575-like), channel slices (ld > C) and the fused epilogues; CASES also holds the layer shapes of
Inception-ResNet-v2 (Mixed_5a .. Bottleneck)."""
import ctypes as C

import numpy as np
import pytest
import torch

from facenet_amd import _lib
from tests.util import (ACC_GRAD_BITS, ACC_STAT_BITS, U_LP, assert_acc_sums, assert_elementwise, bitpattern, conv_desc, conv_fp64, dgrad_fp64,
                        from_acc, gamma, lp_dtype, ptr, ref_conv, rel_err, same_bits, stream, to_acc)

pytestmark = pytest.mark.gpu

CASES = [
    # N, H, W, Cin, Cout, kh, kw, stride, ph, pw
    (2, 19, 19, 8, 32, 3, 3, 2, 0, 0),     # stem 1a-like (Cin padded 3->8)
    (2, 15, 15, 32, 64, 3, 3, 1, 0, 0),    # 2b
    (3, 9, 9, 64, 80, 1, 1, 1, 0, 0),      # 3b (Cout=80)
    (2, 11, 11, 80, 192, 3, 3, 1, 0, 0),   # 4a (Cin=80: K tiles straddle taps)
    (2, 17, 17, 256, 32, 1, 1, 1, 0, 0),   # block35 1x1
    (2, 17, 17, 32, 32, 3, 3, 1, 1, 1),    # block35 3x3 same
    (2, 17, 17, 192, 256, 3, 3, 2, 0, 0),  # reduction stride-2
    (3, 8, 8, 128, 128, 1, 7, 1, 0, 3),    # block17 1x7
    (3, 8, 8, 128, 128, 7, 1, 1, 3, 0),    # block17 7x1
    (5, 3, 3, 192, 192, 1, 3, 1, 0, 1),    # block8 1x3
    (5, 3, 3, 192, 192, 3, 1, 1, 1, 0),    # block8 3x1
    (5, 3, 3, 384, 1792, 1, 1, 1, 0, 0),   # block8 up
    (7, 1, 1, 1792, 128, 1, 1, 1, 0, 0),   # Dense 1792 -> E
    # halo-tile kernel (stride-1 3x3 on maps >= 30x30): ragged 8x16 tiles, partial 32-channel slices, both column-tile widths
    (2, 37, 37, 80, 192, 3, 3, 1, 0, 0),   # 4a at full map size (Cin=80: the third slice is half empty; dgrad: Cout tile 32 x 3)
    (2, 40, 33, 32, 64, 3, 3, 1, 1, 1),    # 'same' padding: zero fill on all four sides
    (1, 45, 39, 32, 32, 3, 3, 1, 0, 0),    # 2a-like: 32-wide column tile
    (2, 35, 35, 192, 80, 3, 3, 1, 0, 0),   # Cout=80 (three 32-wide column tiles, the last half empty), six input slices
    # Inception-ResNet-v2 layer shapes (widths 48, 160, 224, 288, 320, 1088, 2080: 2080 is 32.5 k steps of 64, 16.25 column tiles of 128)
    (2, 17, 17, 48, 64, 5, 5, 1, 2, 2),    # Mixed_5a 5x5 same
    (2, 17, 17, 32, 48, 3, 3, 1, 1, 1),    # block35 0b 3x3 (Cout=48)
    (2, 17, 17, 48, 64, 3, 3, 1, 1, 1),    # block35 0c 3x3 (Cin=48)
    (2, 17, 17, 128, 320, 1, 1, 1, 0, 0),  # block35 up
    (2, 17, 17, 320, 32, 1, 1, 1, 0, 0),   # block35 in
    (2, 17, 17, 320, 384, 3, 3, 2, 0, 0),  # Mixed_6a stride-2
    (3, 8, 8, 1088, 192, 1, 1, 1, 0, 0),   # block17 in
    (3, 8, 8, 128, 160, 1, 7, 1, 0, 3),    # block17 1x7 (Cout=160)
    (3, 8, 8, 160, 192, 7, 1, 1, 3, 0),    # block17 7x1 (Cin=160)
    (3, 8, 8, 384, 1088, 1, 1, 1, 0, 0),   # block17 up
    (3, 8, 8, 256, 288, 3, 3, 2, 0, 0),    # Mixed_7a stride-2 (Cout=288)
    (3, 8, 8, 288, 320, 3, 3, 2, 0, 0),    # Mixed_7a stride-2 (Cin=288)
    (5, 3, 3, 2080, 192, 1, 1, 1, 0, 0),   # block8 in
    (5, 3, 3, 192, 224, 1, 3, 1, 0, 1),    # block8 1x3 (Cout=224)
    (5, 3, 3, 224, 256, 3, 1, 1, 1, 0),    # block8 3x1 (Cin=224)
    (5, 3, 3, 448, 2080, 1, 1, 1, 0, 0),   # block8 up
    (5, 3, 3, 2080, 1536, 1, 1, 1, 0, 0),  # Conv2d_7b
    (7, 1, 1, 1536, 128, 1, 1, 1, 0, 0),   # Bottleneck 1536 -> E
    (1, 35, 35, 32, 48, 3, 3, 1, 1, 1),    # block35 0b 3x3 at 299 pixels: the library itself picks the halo-tile kernel (no request)
]
HALO_CASES = CASES[13:17]
HALO = 9000000      # fn_conv_desc.tile_*: ask for the halo-tile kernel (production picks it only for <= 64 source channels, where it wins)


def _halo(d, case):
    """The halo cases run on conv_halo_kernel whatever the production heuristic would choose (per-descriptor request: the model,
    golden and training tests dispatch exactly like bench.py and users do)."""
    if case in HALO_CASES:
        d.tile_fwd = d.tile_dgrad = HALO
    return d


def test_halo_cases_dispatch_to_the_halo_kernel(lib):
    """The cases above are there to exercise conv_halo_kernel: fn_conv2d_variant reports 9000000 + BN for them (forward and
    data gradient), and an explicit tile sends the same layer to the implicit-GEMM kernel."""
    for (N, H, W, Cin, Cout, kh, kw, s, ph, pw) in HALO_CASES:
        d = conv_desc(N, H, W, Cin, Cout, kh, kw, s, ph, pw, _lib.FN_BF16)
        t = torch.zeros(16, device="cuda")
        d.x = d.w = d.y = d.dx = ptr(t)
        prod = Cin <= 64, Cout <= 64       # the production heuristic: at most 64 SOURCE channels (forward: Cin, data gradient: Cout)
        assert (_lib.variant_is_halo(lib.fn_conv2d_variant(C.byref(d), 0))) == prod[0] and (_lib.variant_is_halo(lib.fn_conv2d_variant(C.byref(d), 1))) == prod[1]
        d.tile_fwd = d.tile_dgrad = HALO
        assert _lib.variant_is_halo(lib.fn_conv2d_variant(C.byref(d), 0)) and _lib.variant_is_halo(lib.fn_conv2d_variant(C.byref(d), 1))
        d.tile_fwd = d.tile_dgrad = 64064
        assert _lib.variant_tile(lib.fn_conv2d_variant(C.byref(d), 0)) == 64064 and _lib.variant_tile(lib.fn_conv2d_variant(C.byref(d), 1)) == 64064   # (+ 2e6: in-launch split-K)
    d = conv_desc(2, 17, 17, 32, 32, 3, 3, 1, 1, 1, _lib.FN_BF16)          # small map: implicit GEMM
    d.x = d.w = d.y = d.dx = ptr(torch.zeros(16, device="cuda"))
    assert not _lib.variant_is_halo(lib.fn_conv2d_variant(C.byref(d), 0))
    d.tile_fwd = HALO                                                       # an explicit request is honoured on any map size ...
    assert _lib.variant_is_halo(lib.fn_conv2d_variant(C.byref(d), 0))
    d = conv_desc(2, 17, 17, 64, 64, 1, 1, 1, 0, 0, _lib.FN_BF16)           # ... but not for a layer the kernel cannot run
    d.x = d.w = d.y = d.dx = ptr(torch.zeros(16, device="cuda"))
    d.tile_fwd = HALO
    assert lib.fn_conv2d_variant(C.byref(d), 0) < 0
    with pytest.raises(_lib.FacenetHipError):
        _lib.check(lib.fn_conv2d_fwd(C.byref(d), stream()))


def _mk(shape, dt, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(lp_dtype(dt)).cuda()


@pytest.mark.parametrize("dt", [_lib.FN_BF16, _lib.FN_F16])
@pytest.mark.parametrize("case", CASES)
def test_conv_fwd(lib, case, dt):
    N, H, W, Cin, Cout, kh, kw, s, ph, pw = case
    x = _mk((N, H, W, Cin), dt, seed=1)
    w = _mk((Cout, kh, kw, Cin), dt, 0.1, seed=2)
    d = _halo(conv_desc(N, H, W, Cin, Cout, kh, kw, s, ph, pw, dt), case)
    y = torch.full((N, d.OH, d.OW, Cout), 7.0, dtype=lp_dtype(dt), device="cuda")
    reps = 4
    stats_r = torch.zeros(reps, 2 * Cout, dtype=torch.int64, device="cuda")      # fixed-point accumulators (fn_acc_t)
    d.x, d.w, d.y, d.stats, d.stats_sq_off, d.stats_replicas, d.stats_rep_stride = ptr(x), ptr(w), ptr(y), ptr(stats_r), Cout, reps, 2 * Cout
    _lib.check(lib.fn_conv2d_fwd(C.byref(d), stream()))
    torch.cuda.synchronize()
    stats = from_acc(stats_r.sum(0), ACC_STAT_BITS)            # row tiles are spread over the accumulator replicas
    first = stats_r.clone()
    for _ in range(2):                 # integer accumulation: the statistics have the same bits every run, in every replica
        stats_r.zero_()
        _lib.check(lib.fn_conv2d_fwd(C.byref(d), stream()))
        torch.cuda.synchronize()
        assert torch.equal(stats_r, first)
    ref = ref_conv(x, w, s, ph, pw)
    assert rel_err(y, ref) < (6e-3 if dt == _lib.FN_BF16 else 8e-4)
    # BatchNorm statistics come from the fp32 accumulators
    M = N * d.OH * d.OW
    s_ref = ref.reshape(M, Cout).sum(0)
    q_ref = (ref.reshape(M, Cout) ** 2).sum(0)
    assert torch.allclose(stats[:Cout].cpu(), s_ref, rtol=2e-3, atol=2e-3 * float(s_ref.abs().max()))
    assert torch.allclose(stats[Cout:].cpu(), q_ref, rtol=2e-3, atol=1e-3)


@pytest.mark.parametrize("dt", [_lib.FN_BF16])
def test_conv_fwd_epilogues_and_slices(lib, dt):
    """bias + residual scale-add + ReLU, output into a channel slice, input from a channel slice, fp32 output."""
    N, H, W, Cin, Cout = 2, 8, 8, 64, 96
    xb = _mk((N, H, W, 160), dt, seed=3)           # input slice [32:96] of a 160-channel buffer
    w = _mk((Cout, 1, 1, Cin), dt, 0.2, seed=4)
    bias = torch.randn(Cout).cuda()
    res = _mk((N, H, W, Cout), dt, seed=5)
    yb = torch.zeros(N, H, W, 256, dtype=lp_dtype(dt), device="cuda")   # output slice [128:224]
    d = conv_desc(N, H, W, Cin, Cout, 1, 1, 1, 0, 0, dt, ld_x=160, ld_y=256)
    d.x, d.w, d.y, d.bias, d.resid, d.ld_res, d.scale, d.relu = ptr(xb, 32), ptr(w), ptr(yb, 128), ptr(bias), ptr(res), Cout, 0.17, 1
    _lib.check(lib.fn_conv2d_fwd(C.byref(d), stream()))
    torch.cuda.synchronize()
    ref = torch.relu(res.float().cpu() + 0.17 * (ref_conv(xb[..., 32:96], w, 1, 0, 0) + bias.cpu()))
    assert rel_err(yb[..., 128:224], ref) < 6e-3
    assert float(yb[..., :128].abs().max()) == 0 and float(yb[..., 224:].abs().max()) == 0   # neighbours untouched
    # fp32 output with a ragged Cout (classifier-like: 203 of 208 columns)
    Cr, Cp = 203, 208
    w2 = _mk((Cp, 1, 1, Cin), dt, 0.2, seed=6)
    w2[Cr:] = 0
    x2 = _mk((5, 1, 1, Cin), dt, seed=7)
    y2 = torch.zeros(5, Cp, dtype=torch.float32, device="cuda")
    d2 = conv_desc(5, 1, 1, Cin, Cp, 1, 1, 1, 0, 0, dt)
    d2.x, d2.w, d2.y, d2.out_f32 = ptr(x2), ptr(w2), ptr(y2), 1
    _lib.check(lib.fn_conv2d_fwd(C.byref(d2), stream()))
    torch.cuda.synchronize()
    assert rel_err(y2.view(5, 1, 1, Cp), ref_conv(x2, w2, 1, 0, 0)) < 1e-5


@pytest.mark.parametrize("dt", [_lib.FN_BF16, _lib.FN_F16])
@pytest.mark.parametrize("case", CASES[1:])
def test_conv_dgrad(lib, case, dt):
    N, H, W, Cin, Cout, kh, kw, s, ph, pw = case
    d = _halo(conv_desc(N, H, W, Cin, Cout, kh, kw, s, ph, pw, dt), case)
    dy = _mk((N, d.OH, d.OW, Cout), dt, seed=11)
    w = _mk((Cout, kh, kw, Cin), dt, 0.1, seed=12)
    wt = torch.zeros_like(w).view(-1)
    table = torch.tensor([[0, Cout, kh * kw * Cin, kh * kw, Cin, -1, -1, 0]], dtype=torch.int32, device="cuda")
    _lib.check(lib.fn_pack_transpose(ptr(w), ptr(wt), ptr(table), 1, w.numel(), dt, stream()))
    dx = torch.full((N, H, W, Cin), 3.0, dtype=lp_dtype(dt), device="cuda")
    d.y, d.w, d.dx = ptr(dy), ptr(wt), ptr(dx)
    _lib.check(lib.fn_conv2d_dgrad(C.byref(d), stream()))
    torch.cuda.synchronize()
    assert torch.equal(wt.view(Cin, kh * kw, Cout).cpu(), w.view(Cout, kh * kw, Cin).permute(2, 1, 0).cpu())
    xr = torch.zeros(N, Cin, H, W, requires_grad=True)
    yr = torch.nn.functional.conv2d(xr, w.float().cpu().permute(0, 3, 1, 2), None, stride=s, padding=(ph, pw))
    yr.backward(dy.float().cpu().permute(0, 3, 1, 2))
    ref = xr.grad.permute(0, 2, 3, 1)
    assert rel_err(dx, ref) < (6e-3 if dt == _lib.FN_BF16 else 8e-4)
    # accumulate mode adds on top
    d.accumulate = 1
    _lib.check(lib.fn_conv2d_dgrad(C.byref(d), stream()))
    torch.cuda.synchronize()
    assert rel_err(dx, 2 * ref) < (1e-2 if dt == _lib.FN_BF16 else 2e-3)


@pytest.mark.parametrize("dt", [_lib.FN_BF16, _lib.FN_F16])
@pytest.mark.parametrize("case", CASES)
def test_conv_wgrad(lib, case, dt):
    N, H, W, Cin, Cout, kh, kw, s, ph, pw = case
    d = conv_desc(N, H, W, Cin, Cout, kh, kw, s, ph, pw, dt)
    x = _mk((N, H, W, Cin), dt, seed=21)
    dy = _mk((N, d.OH, d.OW, Cout), dt, seed=22)
    dw = torch.zeros(Cout, kh, kw, Cin, dtype=torch.float32, device="cuda")
    d.x, d.y, d.dw = ptr(x), ptr(dy), ptr(dw)
    _lib.check(lib.fn_conv2d_wgrad(C.byref(d), stream()))
    torch.cuda.synchronize()
    wr = torch.zeros(Cout, Cin, kh, kw, requires_grad=True)
    yr = torch.nn.functional.conv2d(x.float().cpu().permute(0, 3, 1, 2), wr, None, stride=s, padding=(ph, pw))
    yr.backward(dy.float().cpu().permute(0, 3, 1, 2))
    ref = wr.grad.permute(0, 2, 3, 1)
    assert rel_err(dw, ref) < 2e-5     # operands are exact in low precision, accumulation is fp32
    # forced split-K
    dw.zero_()
    d.splits = 3
    _lib.check(lib.fn_conv2d_wgrad(C.byref(d), stream()))
    torch.cuda.synchronize()
    assert rel_err(dw, ref) < 2e-5


TILE_CASES = [(2, 37, 37, 80, 192, 3, 3, 1, 0, 0),      # 4a: general gather, K tiles straddle taps, 192 = 1.5 x 128 columns
              (2, 35, 35, 192, 256, 3, 3, 2, 0, 0),     # 4b: stride 2 (parity-class data gradient)
              (3, 17, 17, 256, 160, 1, 1, 1, 0, 0),     # 1x1 fast path, ragged rows (867) and a ragged column tile
              (2, 17, 17, 192, 192, 3, 3, 1, 1, 1)]     # 'same' padding


@pytest.mark.parametrize("tile", [128128, 128064, 128032, 64128, 64064, 64032, 32128, 32064, 32032])
@pytest.mark.parametrize("case", TILE_CASES)
def test_conv_explicit_tiles(lib, case, tile):
    """Every tile a caller may pin (fn_conv_desc.tile_fwd / tile_dgrad) gives the convolution, its BatchNorm statistics and the
    data gradient: forward and data gradient against fp32 references on the same rounded operands."""
    dt = _lib.FN_BF16
    N, H, W, Cin, Cout, kh, kw, s, ph, pw = case
    x = _mk((N, H, W, Cin), dt, seed=71)
    w = _mk((Cout, kh, kw, Cin), dt, 0.1, seed=72)
    d = conv_desc(N, H, W, Cin, Cout, kh, kw, s, ph, pw, dt)
    d.tile_fwd = d.tile_dgrad = tile
    assert _lib.variant_tile(lib.fn_conv2d_variant(C.byref(conv_probe(d)), 0)) == tile
    y = torch.zeros(N, d.OH, d.OW, Cout, dtype=lp_dtype(dt), device="cuda")
    reps = 4
    stats_r = torch.zeros(reps, 2 * Cout, dtype=torch.int64, device="cuda")
    d.x, d.w, d.y, d.stats, d.stats_sq_off, d.stats_replicas, d.stats_rep_stride = ptr(x), ptr(w), ptr(y), ptr(stats_r), Cout, reps, 2 * Cout
    _lib.check(lib.fn_conv2d_fwd(C.byref(d), stream()))
    torch.cuda.synchronize()
    ref = ref_conv(x, w, s, ph, pw)
    assert rel_err(y, ref) < 6e-3
    M = N * d.OH * d.OW
    stats = from_acc(stats_r.sum(0), ACC_STAT_BITS).cpu()
    assert torch.allclose(stats[:Cout], ref.reshape(M, Cout).sum(0), rtol=2e-3, atol=2e-3 * float(ref.reshape(M, Cout).sum(0).abs().max()))
    assert torch.allclose(stats[Cout:], (ref.reshape(M, Cout) ** 2).sum(0), rtol=2e-3, atol=1e-3)
    # data gradient
    dy = _mk((N, d.OH, d.OW, Cout), dt, seed=73)
    wt = torch.zeros_like(w).view(-1)
    table = torch.tensor([[0, Cout, kh * kw * Cin, kh * kw, Cin, -1, -1, 0]], dtype=torch.int32, device="cuda")
    _lib.check(lib.fn_pack_transpose(ptr(w), ptr(wt), ptr(table), 1, w.numel(), dt, stream()))
    dx = torch.full((N, H, W, Cin), 3.0, dtype=lp_dtype(dt), device="cuda")
    g = conv_desc(N, H, W, Cin, Cout, kh, kw, s, ph, pw, dt)
    g.tile_dgrad = tile
    g.y, g.w, g.dx = ptr(dy), ptr(wt), ptr(dx)
    _lib.check(lib.fn_conv2d_dgrad(C.byref(g), stream()))
    torch.cuda.synchronize()
    xr = torch.zeros(N, Cin, H, W, requires_grad=True)
    yr = torch.nn.functional.conv2d(xr, w.float().cpu().permute(0, 3, 1, 2), None, stride=s, padding=(ph, pw))
    yr.backward(dy.float().cpu().permute(0, 3, 1, 2))
    assert rel_err(dx, xr.grad.permute(0, 2, 3, 1)) < 6e-3


def conv_probe(d):
    """A copy of the descriptor with dummy pointers where fn_conv2d_variant needs them set."""
    e = _lib.ConvDesc.from_buffer_copy(d)
    e.x = e.w = e.y = e.dx = 4096
    return e


TAPS_CASES = [
    # N, H, W, Cin, Cout, kh, kw, stride, ph, pw, ld_x, ld_y, variant
    (2, 19, 19, 32, 64, 3, 3, 1, 0, 0, 32, 64, 5064090),       # 2b-like, 'valid'
    (2, 17, 17, 32, 32, 3, 3, 1, 1, 1, 96, 32, 5064090),       # block35 3x3 'same', 32 couts, x is a channel slice of a wider buffer
    (2, 37, 37, 80, 192, 3, 3, 1, 0, 0, 80, 192, 5064090),     # 4a: Cin = 80 -> the third 32-channel slice is half empty
    (2, 35, 35, 192, 256, 3, 3, 2, 0, 0, 192, 640, 5064090),   # 4b-like stride 2, dy is a channel slice of a concat buffer
    (2, 17, 17, 256, 384, 3, 3, 2, 0, 0, 256, 384, 5064090),   # reduction_a stride 2 (17 -> 8)
    (3, 8, 8, 128, 128, 1, 7, 1, 0, 3, 128, 128, 5064090),     # block17 1x7
    (3, 8, 8, 128, 128, 7, 1, 1, 3, 0, 128, 256, 5064090),     # block17 7x1
    (1, 45, 39, 32, 40, 3, 3, 1, 1, 1, 32, 40, 5064090),       # ragged tiles, Cout = 40 (one partly empty cout tile)
]


@pytest.mark.parametrize("dt", [_lib.FN_BF16, _lib.FN_F16])
@pytest.mark.parametrize("case", TAPS_CASES)
def test_conv_wgrad_tap_sharing_kernel(lib, case, dt):
    """conv_wgrad_taps_kernel (k x k layers on maps of >= 32 pixels; grouped path only): dW against an fp32 CPU convolution
    gradient on the same rounded operands -- unsplit (direct stores), split over pixels (slabs + ordered reduce), and
    bit-identical from run to run."""
    N, H, W, Cin, Cout, kh, kw, s, ph, pw, ld_x, ld_y, variant = case
    d = conv_desc(N, H, W, Cin, Cout, kh, kw, s, ph, pw, dt, ld_x=ld_x, ld_y=ld_y)
    xb = _mk((N, H, W, ld_x), dt, seed=61)
    dyb = _mk((N, d.OH, d.OW, ld_y), dt, seed=62)
    x0, y0 = (ld_x - Cin) // 2 // 8 * 8, (ld_y - Cout) // 2 // 8 * 8      # the slice starts inside the buffer
    x, dy = xb[..., x0:x0 + Cin], dyb[..., y0:y0 + Cout]
    dw = torch.full((Cout, kh, kw, Cin), float("nan"), dtype=torch.float32, device="cuda")
    d.x, d.y, d.dw = ptr(xb, x0), ptr(dyb, y0), ptr(dw)
    assert lib.fn_conv2d_variant(C.byref(d), 2) == variant
    wr = torch.zeros(Cout, Cin, kh, kw, requires_grad=True)
    yr = torch.nn.functional.conv2d(x.float().cpu().permute(0, 3, 1, 2), wr, None, stride=s, padding=(ph, pw))
    yr.backward(dy.float().cpu().permute(0, 3, 1, 2))
    ref = wr.grad.permute(0, 2, 3, 1)
    nbytes = lib.fn_conv2d_wgrad_arg_bytes()
    for splits in (1, 3, 0):                       # 0: the library's own choice
        d.splits = splits
        arr = (_lib.ConvDesc * 1)(d)
        host_args, host_prefix, ws_elems = (C.c_uint8 * nbytes)(), (C.c_int32 * 2)(), C.c_int64(0)
        total = lib.fn_conv2d_wgrad_group_build(arr, 1, variant, host_args, host_prefix, None, C.byref(ws_elems))
        nslabs = ws_elems.value // dw.numel()        # a layer cannot be split into more pieces than it has pixel tiles
        assert total > 0 and ws_elems.value % dw.numel() == 0 and (splits != 1 or nslabs == 0) and (splits != 3 or 2 <= nslabs <= 3)
        ws = torch.full((max(1, ws_elems.value),), float("nan"), device="cuda")
        total = lib.fn_conv2d_wgrad_group_build(arr, 1, variant, host_args, host_prefix, ptr(ws), C.byref(ws_elems))
        dev_args = torch.frombuffer(bytearray(host_args), dtype=torch.uint8).cuda()
        dev_prefix = torch.tensor(list(host_prefix), dtype=torch.int32, device="cuda")
        runs = []
        for _ in range(2):
            dw.fill_(float("nan"))
            _lib.check(lib.fn_conv2d_wgrad_grouped(ptr(dev_args), ptr(dev_prefix), 1, total, variant, dt, stream()))
            _lib.check(lib.fn_conv2d_wgrad_reduce(ptr(dev_args), 1, stream()))
            torch.cuda.synchronize()
            runs.append(dw.clone())
        assert rel_err(runs[0], ref) < 2e-5, splits
        assert torch.equal(runs[0], runs[1])
    # the single-layer launch of the same descriptor (general kernel, atomics) agrees
    d.splits = 0
    dw.zero_()
    _lib.check(lib.fn_conv2d_wgrad(C.byref(d), stream()))
    torch.cuda.synchronize()
    assert rel_err(dw, runs[0]) < 2e-5
    # layers the kernel does not take: 3x3 maps, fewer than 32 input channels, 1x1
    for (hh, cin, k) in ((3, 192, 3), (19, 8, 3), (17, 64, 1)):
        e = conv_desc(2, hh, hh, cin, 64, k, k, 1, k // 2, k // 2, dt)
        e.x = e.y = e.dw = ptr(dw)
        assert not _lib.variant_is_taps(lib.fn_conv2d_variant(C.byref(e), 2))


def test_conv_rejects_bad_geometry(lib):
    d = conv_desc(1, 8, 8, 12, 16, 3, 3, 1, 0, 0, _lib.FN_BF16)   # Cin not a multiple of 8
    x = torch.zeros(1, 8, 8, 12, dtype=torch.bfloat16, device="cuda")
    d.x = d.w = d.y = ptr(x)
    with pytest.raises(ValueError):
        _lib.check(lib.fn_conv2d_fwd(C.byref(d), stream()))


def test_conv_wgrad_grouped_matches_single_launches(lib):
    """fn_conv2d_wgrad_grouped: several layers of one tile variant in ONE launch == the per-layer launches."""
    dt = _lib.FN_BF16
    cases = [(3, 8, 8, 128, 128, 1, 7, 1, 0, 3), (3, 8, 8, 896, 128, 1, 1, 1, 0, 0), (2, 17, 17, 192, 192, 3, 3, 1, 1, 1),
             (5, 3, 3, 192, 192, 3, 1, 1, 1, 0), (2, 17, 17, 192, 256, 3, 3, 2, 0, 0),
             # second and third members for every tap-sharing variant (records of a group are fn_conv2d_wgrad_arg_bytes() apart)
             (2, 19, 19, 64, 64, 3, 3, 1, 0, 0), (1, 33, 21, 96, 128, 3, 3, 1, 1, 1), (2, 17, 17, 64, 96, 3, 3, 2, 0, 0),
             (3, 8, 8, 128, 128, 7, 1, 1, 3, 0), (2, 9, 12, 64, 80, 1, 7, 1, 0, 3), (4, 17, 17, 256, 32, 1, 1, 1, 0, 0)]
    descs, keep, singles = [], [], []
    for i, (N, H, W, Cin, Cout, kh, kw, s, ph, pw) in enumerate(cases):
        d = conv_desc(N, H, W, Cin, Cout, kh, kw, s, ph, pw, dt)
        x = _mk((N, H, W, Cin), dt, seed=31 + i)
        dy = _mk((N, d.OH, d.OW, Cout), dt, seed=41 + i)
        dw = torch.zeros(Cout, kh, kw, Cin, dtype=torch.float32, device="cuda")
        ref = torch.zeros_like(dw)
        d.x, d.y, d.dw = ptr(x), ptr(dy), ptr(ref)
        _lib.check(lib.fn_conv2d_wgrad(C.byref(d), stream()))
        d.dw = ptr(dw)
        descs.append(d); keep.append((x, dy, dw, ref))
    groups = {}
    for d, k in zip(descs, keep):
        groups.setdefault(lib.fn_conv2d_variant(C.byref(d), 2), []).append((d, k))
    assert len(groups) >= 1 and [len(m) for v, m in groups.items() if _lib.variant_is_taps(v)] == [8]
    nbytes = lib.fn_conv2d_wgrad_arg_bytes()
    for variant, members in groups.items():
        n = len(members)
        arr = (_lib.ConvDesc * n)(*[m[0] for m in members])
        host_args = (C.c_uint8 * (nbytes * n))()
        host_prefix = (C.c_int32 * (n + 1))()
        ws_elems = C.c_int64(0)
        assert lib.fn_conv2d_wgrad_group_build(arr, n, variant, host_args, host_prefix, None, C.byref(ws_elems)) > 0     # sizing call
        ws = torch.full((max(1, ws_elems.value),), float("nan"), device="cuda")           # every slab element must be written
        total = lib.fn_conv2d_wgrad_group_build(arr, n, variant, host_args, host_prefix, ptr(ws), C.byref(ws_elems))
        assert total > 0 and list(host_prefix)[0] == 0 and list(host_prefix)[-1] == total
        dev_args = torch.frombuffer(bytearray(host_args), dtype=torch.uint8).cuda()
        dev_prefix = torch.tensor(list(host_prefix), dtype=torch.int32, device="cuda")
        for _, k in members:
            k[2].fill_(float("nan"))                                                       # dw needs no zeroing on the grouped path
        _lib.check(lib.fn_conv2d_wgrad_grouped(ptr(dev_args), ptr(dev_prefix), n, total, variant, dt, stream()))
        _lib.check(lib.fn_conv2d_wgrad_reduce(ptr(dev_args), n, stream()))
        torch.cuda.synchronize()
        first = [k[2].clone() for _, k in members]
        assert not any(bool(torch.isnan(f).any()) for f in first)
        for _ in range(3):                      # atomic-free, fixed summation order: the same bits every run
            _lib.check(lib.fn_conv2d_wgrad_grouped(ptr(dev_args), ptr(dev_prefix), n, total, variant, dt, stream()))
            _lib.check(lib.fn_conv2d_wgrad_reduce(ptr(dev_args), n, stream()))
            torch.cuda.synchronize()
            assert all(torch.equal(f, k[2]) for f, (_, k) in zip(first, members))
    torch.cuda.synchronize()
    for (x, dy, dw, ref) in keep:
        assert rel_err(dw, ref) < 2e-5
    # a descriptor of another variant is rejected
    bad = (_lib.ConvDesc * 1)(descs[0])
    other = [v for v in (32064, 64064, 128128) if v != lib.fn_conv2d_variant(C.byref(descs[0]), 2)][0]
    with pytest.raises(ValueError):
        _lib.check(lib.fn_conv2d_wgrad_group_build(bad, 1, other, (C.c_uint8 * nbytes)(), (C.c_int32 * 2)(), None, C.byref(C.c_int64(0))))


@pytest.mark.parametrize("dt", [_lib.FN_BF16, _lib.FN_F16])
@pytest.mark.parametrize("H", [17, 37])           # 37: the halo-tile kernel runs the same shared epilogue
def test_dgrad_fused_bn_backward_reduction(lib, dt, H):
    """dgrad epilogue computing sum(dyh) / sum(dyh*xhat) of the producing layer's BatchNorm (+ReLU) == the standalone
    reduce kernel; the apply kernel then consumes the replicated accumulators."""
    N, W, Cin, Cout = 3, H, 64, 96
    d = conv_desc(N, H, W, Cin, Cout, 3, 3, 1, 1, 1, dt)
    if H == 37:
        d.tile_dgrad = HALO          # 96 source channels: production would take the implicit-GEMM kernel
    M = N * H * W
    dy = _mk((N, H, W, Cout), dt, seed=51)
    w = _mk((Cout, 3, 3, Cin), dt, 0.1, seed=52)
    wt = torch.zeros_like(w).view(-1)
    table = torch.tensor([[0, Cout, 9 * Cin, 9, Cin, -1, -1, 0]], dtype=torch.int32, device="cuda")
    _lib.check(lib.fn_pack_transpose(ptr(w), ptr(wt), ptr(table), 1, w.numel(), dt, stream()))
    yraw = _mk((N, H, W, Cin), dt, seed=53, scale=2.0)
    beta = (torch.randn(Cin, generator=torch.Generator().manual_seed(54)) * 0.3).cuda()
    yf = yraw.float().view(M, Cin)
    mean, var = yf.mean(0), yf.var(0, unbiased=False)
    sc = torch.rsqrt(var + 1e-3).contiguous()
    sh = (beta - mean * sc).contiguous()
    reps = 4
    acc = torch.zeros(reps, 2 * Cin, dtype=torch.int64, device="cuda")      # fixed point, FN_ACC_GRAD_BITS
    dx = torch.zeros(N, H, W, Cin, dtype=lp_dtype(dt), device="cuda")
    d.y, d.w, d.dx = ptr(dy), ptr(wt), ptr(dx)
    d.bn_y, d.ld_bn_y, d.bn_scale, d.bn_shift, d.bn_beta = ptr(yraw), Cin, ptr(sc), ptr(sh), ptr(beta)
    d.bn_acc, d.bn_sq_off, d.bn_replicas, d.bn_rep_stride, d.bn_relu = ptr(acc), Cin, reps, 2 * Cin, 1
    assert (_lib.variant_is_halo(lib.fn_conv2d_variant(C.byref(d), 1))) == (H == 37)
    _lib.check(lib.fn_conv2d_dgrad(C.byref(d), stream()))
    # reference: standalone reduce on the (rounded) dx
    acc_ref = torch.zeros(2 * Cin, dtype=torch.int64, device="cuda")
    dbeta_ref = torch.zeros(Cin, device="cuda")
    dx_ref = dx.clone()
    _lib.check(lib.fn_bn_relu_train_bwd(ptr(dx_ref), Cin, ptr(yraw), Cin, M, Cin, ptr(beta), ptr(sc), ptr(sh), ptr(dbeta_ref), ptr(acc_ref), Cin, 1, 0,
                                        0, 1, dt, stream()))
    dbeta = torch.zeros(Cin, device="cuda")
    _lib.check(lib.fn_bn_relu_train_bwd(ptr(dx), Cin, ptr(yraw), Cin, M, Cin, ptr(beta), ptr(sc), ptr(sh), ptr(dbeta), ptr(acc), Cin, reps, 2 * Cin,
                                        1, 1, dt, stream()))
    torch.cuda.synchronize()
    tol = 2e-2 if dt == _lib.FN_BF16 else 3e-3       # fused sums use the un-rounded fp32 gradient
    assert rel_err(from_acc(acc.sum(0), ACC_GRAD_BITS), from_acc(acc_ref, ACC_GRAD_BITS)) < tol
    assert rel_err(dbeta, dbeta_ref) < tol
    assert rel_err(dx, dx_ref) < tol


NORM_CASES = [c for c in CASES if c[3] <= 512 and c[3] >= 32]


@pytest.mark.parametrize("dt", [_lib.FN_BF16, _lib.FN_F16])
@pytest.mark.parametrize("case", NORM_CASES)
def test_conv_normalise_on_load_equals_materialised_bn(lib, case, dt):
    """fwd and wgrad with nrm_* on the RAW tensor must give exactly what they give on the tensor fn_bn_relu_train_fwd writes
    (same statistics, same rounding of the activated operand), including zero padding and channel slices."""
    N, H, W, Cin, Cout, kh, kw, s, ph, pw = case
    M = N * H * W
    ld = Cin + 16                                      # x is the slice [8, 8+Cin) of a wider buffer
    raw = _mk((N, H, W, ld), dt, 1.5, seed=11)
    rawf = raw[..., 8:8 + Cin].float().reshape(M, Cin)
    reps, CBs = 4, Cin + 24                            # statistics live at offset 16 of a wider channel space
    stats = torch.zeros(reps, 2 * CBs, dtype=torch.int64, device="cuda")
    part = torch.arange(M, device="cuda") % reps
    for r in range(reps):                              # replicas hold partial sums (fixed point), as the producing conv leaves them
        stats[r, 16:16 + Cin] = to_acc(rawf[part == r].sum(0), ACC_STAT_BITS)
        stats[r, CBs + 16:CBs + 16 + Cin] = to_acc((rawf[part == r] ** 2).sum(0), ACC_STAT_BITS)
    beta = (torch.randn(CBs, generator=torch.Generator().manual_seed(5)) * 0.3).cuda()
    z = torch.zeros_like(raw)
    sc, sh = torch.zeros(CBs, device="cuda"), torch.zeros(CBs, device="cuda")
    _lib.check(lib.fn_bn_relu_train_fwd(ptr(raw, 8), ld, ptr(z, 8), ld, M, Cin, ptr(stats, 16), CBs, reps, 2 * CBs, ptr(beta, 16),
                                        ptr(sc, 16), ptr(sh, 16), None, None, 0.99, 1e-3, 1, dt, stream()))
    w = _mk((Cout, kh, kw, Cin), dt, 0.1, seed=12)
    outs = []
    for norm in (False, True):
        d = conv_desc(N, H, W, Cin, Cout, kh, kw, s, ph, pw, dt, ld_x=ld)
        y = torch.zeros(N, d.OH, d.OW, Cout, dtype=lp_dtype(dt), device="cuda")
        d.w, d.y = ptr(w), ptr(y)
        if norm:
            d.x, d.nrm_stats, d.nrm_beta = ptr(raw, 8), ptr(stats, 16), ptr(beta, 16)
            d.nrm_sq_off, d.nrm_replicas, d.nrm_rep_stride, d.nrm_count, d.nrm_eps = CBs, reps, 2 * CBs, M, 1e-3
        else:
            d.x = ptr(z, 8)
        _lib.check(lib.fn_conv2d_fwd(C.byref(d), stream()))
        dy = _mk((N, d.OH, d.OW, Cout), dt, seed=13)
        dw = torch.zeros(Cout, kh * kw * Cin, dtype=torch.float32, device="cuda")
        d.y, d.dw, d.splits = ptr(dy), ptr(dw), 1      # one split: the accumulation order is fixed, results comparable bit for bit
        _lib.check(lib.fn_conv2d_wgrad(C.byref(d), stream()))
        torch.cuda.synchronize()
        outs.append((y, dw))
    # operands are bit-identical; the plain launch may use in-launch split-K (another summation order), the nrm one never does
    assert rel_err(outs[1][0], outs[0][0]) < (2e-3 if dt == _lib.FN_BF16 else 3e-4)
    assert torch.equal(outs[0][1], outs[1][1])
    assert float(outs[0][0].float().abs().max()) > 0 and float(outs[0][1].abs().max()) > 0
    # fn_bn_finalize publishes the same scale / shift and moving statistics as the materialising kernel
    sc2, sh2 = torch.zeros(CBs, device="cuda"), torch.zeros(CBs, device="cuda")
    mm, mv = torch.zeros(CBs, device="cuda"), torch.ones(CBs, device="cuda")
    mm_ref, mv_ref = torch.zeros(CBs, device="cuda"), torch.ones(CBs, device="cuda")
    _lib.check(lib.fn_bn_relu_train_fwd(ptr(raw, 8), ld, ptr(z, 8), ld, M, Cin, ptr(stats, 16), CBs, reps, 2 * CBs, ptr(beta, 16),
                                        ptr(sc, 16), ptr(sh, 16), ptr(mm_ref, 16), ptr(mv_ref, 16), 0.99, 1e-3, 1, dt, stream()))
    fr = torch.zeros(CBs, dtype=torch.int32, device="cuda")
    fr[16:16 + Cin] = reps
    fc = torch.full((CBs,), M, dtype=torch.int32, device="cuda")
    _lib.check(lib.fn_bn_finalize(ptr(stats), CBs, 2 * CBs, ptr(fr), ptr(fc), ptr(beta), ptr(sc2), ptr(sh2), ptr(mm), ptr(mv), 0.99, 1e-3, CBs,
                                  stream()))
    torch.cuda.synchronize()
    assert torch.equal(sc, sc2) and torch.equal(sh, sh2) and torch.equal(mm, mm_ref) and torch.equal(mv, mv_ref)
    assert float(sc2[:16].abs().max()) == 0 and float(sc2[16 + Cin:].abs().max()) == 0      # channels with reps == 0 untouched


def test_conv_normalise_on_load_rejects_wide_inputs(lib):
    d = conv_desc(1, 3, 3, 1792, 128, 1, 1, 1, 0, 0, _lib.FN_BF16)
    x = torch.zeros(1, 3, 3, 1792, dtype=torch.bfloat16, device="cuda")
    w = torch.zeros(128, 1, 1, 1792, dtype=torch.bfloat16, device="cuda")
    y = torch.zeros(1, 3, 3, 128, dtype=torch.bfloat16, device="cuda")
    st = torch.zeros(2 * 1792, dtype=torch.int64, device="cuda")
    d.x, d.w, d.y, d.nrm_stats, d.nrm_beta, d.nrm_count, d.nrm_eps, d.nrm_sq_off = ptr(x), ptr(w), ptr(y), ptr(st), ptr(st), 9, 1e-3, 1792
    with pytest.raises(ValueError):
        _lib.check(lib.fn_conv2d_fwd(C.byref(d), stream()))


@pytest.mark.parametrize("dt", [_lib.FN_BF16, _lib.FN_F16])
@pytest.mark.parametrize("nsrc", [2, 3])
@pytest.mark.parametrize("tile", [0, 128064, 64064, 32032, 32128])
def test_dgrad_sibling_sources_equal_the_sum_of_single_dgrads(lib, dt, nsrc, tile):
    """dX of 2-3 sibling 1x1 layers as ONE multi-source launch (dy2/w2, dy3/w3, own row strides and widths, K tails that are
    not multiples of the 64-wide k tile) == the fp32 sum of the per-layer products, with and without accumulation."""
    N, H, W, Cin = 3, 9, 9, 256
    couts, lds = [32, 40, 96][:nsrc], [96, 40, 160][:nsrc]          # dY slices of wider buffers (ld > Cout) like `mixed`
    M = N * H * W
    dys = [_mk((N, H, W, ld), dt, seed=20 + i) for i, ld in enumerate(lds)]
    wts = [_mk((Cin, 1, 1, c), dt, 0.1, seed=30 + i) for i, c in enumerate(couts)]      # transposed packs [Cin][tap][Cout]
    ref = sum(dy[..., :c].float().cpu().reshape(M, c) @ wt.float().cpu().reshape(Cin, c).t() for dy, wt, c in zip(dys, wts, couts))
    d = conv_desc(N, H, W, Cin, couts[0], 1, 1, 1, 0, 0, dt, ld_y=lds[0])
    d.tile_dgrad = tile
    d.y, d.w = ptr(dys[0]), ptr(wts[0])
    d.dy2, d.w2, d.Cout2, d.ld_y2 = ptr(dys[1]), ptr(wts[1]), couts[1], lds[1]
    if nsrc == 3:
        d.dy3, d.w3, d.Cout3, d.ld_y3 = ptr(dys[2]), ptr(wts[2]), couts[2], lds[2]
    dx = torch.full((N, H, W, Cin), 3.0, dtype=lp_dtype(dt), device="cuda")
    d.dx = ptr(dx)
    _lib.check(lib.fn_conv2d_dgrad(C.byref(d), stream()))
    torch.cuda.synchronize()
    tol = 6e-3 if dt == _lib.FN_BF16 else 8e-4
    assert rel_err(dx.reshape(M, Cin), ref) < tol
    base = dx.float().cpu().reshape(M, Cin).clone()
    d.accumulate = 1
    _lib.check(lib.fn_conv2d_dgrad(C.byref(d), stream()))
    torch.cuda.synchronize()
    assert rel_err(dx.reshape(M, Cin), base + ref) < 2 * tol
    d.Cout2 = 33                                                    # not a multiple of 8
    with pytest.raises(ValueError):
        _lib.check(lib.fn_conv2d_dgrad(C.byref(d), stream()))


# ---- element-wise bounds: grouped launches, the fused residual backward, every tile / split-K variant ------------------------
# References are fp64 on the CPU from the operands the kernel reads; tests.util.assert_elementwise holds EVERY element to the
# worst-case fp32-accumulation bound plus one rounding to the storage type, tests.util.assert_acc_sums the fixed-point sums.
# Outputs start as NaN, bytes a launch must not touch hold tests.util.bitpattern and are compared bit for bit afterwards.

def _pack_t(lib, w, dt):
    """Transposed pack [Cin][tap][Cout] of w [Cout][kh][kw][Cin] (what the data gradient reads)."""
    Cout, kh, kw, Cin = w.shape
    wt = torch.zeros_like(w).view(-1)
    table = torch.tensor([[0, Cout, kh * kw * Cin, kh * kw, Cin, -1, -1, 0]], dtype=torch.int32, device="cuda")
    _lib.check(lib.fn_pack_transpose(ptr(w), ptr(wt), ptr(table), 1, w.numel(), dt, stream()))
    return wt


class _Buf:
    """Low-precision buffer: claimed channel slices start as NaN (or a given base), everything else as a fixed bit pattern."""

    def __init__(self, shape, dt):
        self.t = torch.empty(shape, dtype=lp_dtype(dt), device="cuda")
        self.init = bitpattern(shape, dt)
        self.free = torch.ones(shape[-1], dtype=torch.bool, device="cuda")

    def claim(self, c0, c, base=None):
        assert bool(self.free[c0:c0 + c].all())
        self.free[c0:c0 + c] = False
        self.init[..., c0:c0 + c] = float("nan") if base is None else base

    def reset(self):
        self.t.copy_(self.init)

    def check_untouched(self, what):
        assert same_bits(self.t[..., self.free], self.init[..., self.free]), f"{what}: bytes outside the written slices changed"


class _Acc:
    """Fixed-point accumulators [replicas][2 * CB] (sum | sum of squares), zero outside the claimed columns."""

    def __init__(self, reps, CB):
        self.t = torch.zeros(reps, 2 * CB, dtype=torch.int64, device="cuda")
        self.CB = CB
        self.free = torch.ones(reps, 2 * CB, dtype=torch.bool, device="cuda")

    def claim(self, off, c, reps, sq=True):
        for o in ((off, off + self.CB) if sq else (off,)):
            assert bool(self.free[:reps, o:o + c].all())
            self.free[:reps, o:o + c] = False

    def reset(self):
        self.t.zero_()

    def check_untouched(self, what):
        assert int(self.t[self.free].abs().sum()) == 0, f"{what}: accumulators outside the claimed columns changed"


def _geo(geo):
    N, H, W, Cin, Cout, kh, kw, s, ph, pw = geo
    return N, H, W, Cin, Cout, kh, kw, s, ph, pw, (H + 2 * ph - kh) // s + 1, (W + 2 * pw - kw) // s + 1


def _tiles(M):
    return (M + 31) // 32 + 4          # workgroups that can add into one column of a fixed-point sum (any tile, parity classes)


_MEMO = {}


def _memo(key, make):
    """fp64 references of operands that are a function of `key` alone, shared between the tests that follow each other (the
    tiles of one layer); a handful are kept."""
    if key not in _MEMO:
        while len(_MEMO) >= 8:
            _MEMO.pop(next(iter(_MEMO)))
        _MEMO[key] = make()
    return _MEMO[key]


class _Layer:
    """One convolution launch (forward op 0 / data gradient op 1) with its fp64 reference and its checks."""

    def __init__(self, op, d, keep, checks, bufs):
        self.op, self.d, self.keep, self.checks, self.bufs = op, d, keep, checks, bufs

    def launch(self, lib):
        _lib.check((lib.fn_conv2d_fwd if self.op == 0 else lib.fn_conv2d_dgrad)(C.byref(self.d), stream()))

    def check(self, what):
        for c in self.checks:
            c(what)


def _fwd_layer(lib, dt, geo, seed, out, c0=0, x=None, x_c0=0, stats=None, bias=False, resid=False, scale=1.0, relu=0, tile=0):
    """out: _Buf receiving channels [c0, c0 + Cout); x: shared input buffer (channels [x_c0, x_c0 + Cin)); stats: (_Acc, offset, replicas)."""
    N, H, W, Cin, Cout, kh, kw, s, ph, pw, OH, OW = _geo(geo)
    fresh = x is None
    if fresh:
        x = _mk((N, H, W, Cin), dt, seed=seed)
    w = _mk((Cout, kh, kw, Cin), dt, 0.1, seed=seed + 1)
    d = conv_desc(N, H, W, Cin, Cout, kh, kw, s, ph, pw, dt, ld_x=x.shape[-1], ld_y=out.t.shape[-1])
    d.x, d.w, d.y, d.relu, d.tile_fwd = ptr(x, x_c0), ptr(w), ptr(out.t, c0), relu, tile
    out.claim(c0, Cout)
    # operands made here are a function of (geo, dt, seed): their reference is computed once and shared (never modified)
    conv, aconv = _memo(("fwd", geo, dt, seed), lambda: conv_fp64(x, w, s, ph, pw)) if fresh else conv_fp64(x[..., x_c0:x_c0 + Cin], w, s, ph, pw)
    ref, aref, keep = conv, aconv, [x, w]
    if bias:
        b = (torch.randn(Cout, generator=torch.Generator().manual_seed(seed + 2)) * 0.5).cuda()
        d.bias = ptr(b)
        keep.append(b)
        ref, aref = ref + b.double().cpu(), aref + b.double().abs().cpu()
    if resid:
        r = _mk((N, OH, OW, Cout), dt, seed=seed + 3)
        d.resid, d.ld_res, d.scale = ptr(r), Cout, scale
        keep.append(r)
        ref, aref = r.double().cpu() + scale * ref, r.double().abs().cpu() + abs(scale) * aref
    if relu:
        ref = ref.clamp_min(0)
    K = kh * kw * Cin
    checks = [lambda what: assert_elementwise(out.t[..., c0:c0 + Cout], ref, aref, K + 3, dt, what + ": y")]
    bufs = [out]
    if stats is not None:
        acc, off, reps = stats
        acc.claim(off, Cout, reps)
        d.stats, d.stats_sq_off, d.stats_replicas, d.stats_rep_stride = ptr(acc.t, off), acc.CB, reps, 2 * acc.CB
        bufs.append(acc)
        M = N * OH * OW
        y, e = conv.reshape(M, Cout), gamma(K) * aconv.reshape(M, Cout)       # the un-rounded fp32 accumulators and their error

        def chk_stats(what):
            s_, q_ = acc.t[:, off:off + Cout].sum(0), acc.t[:, acc.CB + off:acc.CB + off + Cout].sum(0)
            assert_acc_sums(s_, y.sum(0), y.abs().sum(0), ACC_STAT_BITS, _tiles(M), what + ": sum", term_err=e.sum(0))
            qe = 2 * y.abs() * e + e * e + 2.0 ** -24 * (y.abs() + e) ** 2
            assert_acc_sums(q_, (y * y).sum(0), (y * y).sum(0), ACC_STAT_BITS, _tiles(M), what + ": sum of squares", term_err=qe.sum(0))
        checks.append(chk_stats)
    return _Layer(0, d, keep, checks, bufs)


def _dgrad_layer(lib, dt, geo, seed, out, c0=0, accumulate=0, bn=None, tile=0, siblings=(), rb=None, lds=None):
    """out: _Buf receiving dX channels [c0, c0 + Cin); accumulate: dX adds to a random base; bn: (_Acc, offset, replicas, relu)
    for the fused BatchNorm-backward reduction of the layer that produced x; siblings: Cout of the 1x1 sources dy2 / dy3;
    rb: the fused residual backward (see _fuse_rb); lds: row strides of dy, dy2, dy3 (each source the first channels of a wider
    buffer, like the slices of `mixed`; default: contiguous)."""
    N, H, W, Cin, Cout, kh, kw, s, ph, pw, OH, OW = _geo(geo)
    lds = list(lds) if lds else [Cout] + list(siblings)
    dyb = _mk((N, OH, OW, lds[0]), dt, seed=seed)
    dy = dyb[..., :Cout]
    w = _mk((Cout, kh, kw, Cin), dt, 0.1, seed=seed + 1)
    wt = _pack_t(lib, w, dt)
    d = conv_desc(N, H, W, Cin, Cout, kh, kw, s, ph, pw, dt, ld_x=out.t.shape[-1], ld_y=lds[0])
    d.y, d.w, d.dx, d.accumulate, d.tile_dgrad = ptr(dyb), ptr(wt), ptr(out.t, c0), accumulate, tile
    g, ag = _memo(("dgrad", geo, dt, seed, lds[0]), lambda: dgrad_fp64(dy, w, H, W, s, ph, pw))
    ref, aref, keep = g, ag, [dyb, w, wt]
    K = kh * kw * Cout
    for i, c2 in enumerate(siblings):          # sibling 1x1 layers reading the same x: their products join the same GEMM
        dyib, wi = _mk((N, OH, OW, lds[1 + i]), dt, seed=seed + 10 + i), _mk((c2, 1, 1, Cin), dt, 0.1, seed=seed + 20 + i)
        dyi = dyib[..., :c2]
        wti = _pack_t(lib, wi, dt)
        setattr(d, ("dy2", "dy3")[i], ptr(dyib)); setattr(d, ("w2", "w3")[i], ptr(wti))
        setattr(d, ("Cout2", "Cout3")[i], c2); setattr(d, ("ld_y2", "ld_y3")[i], lds[1 + i])
        gi, agi = _memo(("sibling", geo[:4], c2, dt, seed, i, lds[1 + i]), lambda: dgrad_fp64(dyi, wi, H, W, 1, 0, 0))
        ref, aref, K = ref + gi, aref + agi, K + c2
        keep += [dyib, wi, wti]
    if rb is not None:
        return _fuse_rb(lib, dt, d, out, c0, ref, aref, K, seed, keep, **rb)
    if accumulate:
        base = _mk((N, H, W, Cin), dt, seed=seed + 2)
        out.claim(c0, Cin, base)
        ref, aref = ref + base.double().cpu(), aref + base.double().abs().cpu()
    else:
        out.claim(c0, Cin)
    checks = [lambda what: assert_elementwise(out.t[..., c0:c0 + Cin], ref, aref, K + 2, dt, what + ": dx")]
    bufs = [out]
    if bn is not None:
        acc, off, reps, relu = bn
        acc.claim(off, Cin, reps)
        M = N * H * W
        yraw = _mk((N, H, W, Cin), dt, seed=seed + 3, scale=2.0)
        gen = torch.Generator().manual_seed(seed + 4)
        sc = (torch.rand(Cin, generator=gen) + 0.5).cuda()
        sh = (torch.randn(Cin, generator=gen) * 0.5).cuda()
        beta = (torch.randn(Cin, generator=gen) * 0.3).cuda()
        d.bn_y, d.ld_bn_y, d.bn_scale, d.bn_shift, d.bn_beta = ptr(yraw), Cin, ptr(sc), ptr(sh), ptr(beta)
        d.bn_acc, d.bn_sq_off, d.bn_replicas, d.bn_rep_stride, d.bn_relu = ptr(acc.t, off), acc.CB, reps, 2 * acc.CB, relu
        keep += [yraw, sc, sh, beta]
        bufs.append(acc)
        z = yraw.double().cpu().reshape(M, Cin) * sc.double().cpu() + sh.double().cpu()      # fma(y, scale, shift) before its rounding
        keep_m = (z > 0).double() if relu else torch.ones_like(z)
        gm, e = g.reshape(M, Cin) * keep_m, gamma(K) * ag.reshape(M, Cin) * keep_m         # the un-rounded fp32 gradient
        zb = z - beta.double().cpu()
        zab = z.abs() + beta.double().abs().cpu()
        u = 2.0 ** -24

        def chk_bn(what):
            s_, q_ = acc.t[:, off:off + Cin].sum(0), acc.t[:, acc.CB + off:acc.CB + off + Cin].sum(0)
            assert_acc_sums(s_, gm.sum(0), gm.abs().sum(0), ACC_GRAD_BITS, _tiles(M), what + ": sum dyh", term_err=e.sum(0))
            qe = e * zab + (gm.abs() + e) * 4 * u * zab
            assert_acc_sums(q_, (gm * zb).sum(0), (gm * zb).abs().sum(0), ACC_GRAD_BITS, _tiles(M), what + ": sum dyh*xhat", term_err=qe.sum(0))
        checks.append(chk_bn)
    return _Layer(1, d, keep, checks, bufs)


def _plain_bits(d, op):
    return int(d.KH == 1 and d.KW == 1 and d.stride == 1 and d.pad_h == 0 and d.pad_w == 0) | (2 if op == 0 and d.nrm_stats else 0)


def _group(lib, layers, dt):
    """The grouped launch train.group_convs builds for these layers: records of fn_conv2d_arg_bytes(), the prefix array and
    the LDS size fn_conv2d_group_build returns."""
    n, op = len(layers), layers[0].op
    variant = lib.fn_conv2d_variant(C.byref(layers[0].d), op)
    assert all(lib.fn_conv2d_variant(C.byref(L.d), op) == variant for L in layers), [lib.fn_conv2d_variant(C.byref(L.d), op) for L in layers]
    plain = _plain_bits(layers[0].d, op)
    descs = (_lib.ConvDesc * n)(*[L.d for L in layers])
    host_args, host_prefix, smem = (C.c_uint8 * (lib.fn_conv2d_arg_bytes() * n))(), (C.c_int32 * (n + 1))(), C.c_int32(0)
    total = lib.fn_conv2d_group_build(descs, n, op, variant, host_args, host_prefix, C.byref(smem))
    if total < 0:
        _lib.check(total, "conv_group_build")
    prefix = list(host_prefix)
    assert prefix[0] == 0 and prefix[-1] == total and all(b > a for a, b in zip(prefix, prefix[1:]))
    dev_args = torch.frombuffer(bytearray(host_args), dtype=torch.uint8).cuda()
    dev_prefix = torch.tensor(prefix, dtype=torch.int32, device="cuda")

    def run():
        _lib.check(lib.fn_conv2d_grouped(ptr(dev_args), ptr(dev_prefix), n, total, variant, plain, smem.value, dt, stream()))
    return run, variant, prefix


def _check_group(lib, layers, dt, what):
    """Single launches, then the grouped launch twice: every buffer bit-equal, every layer within the element-wise bound, bytes
    outside the layers' slices untouched.  Returns (variant, prefix)."""
    bufs = list({id(b): b for L in layers for b in L.bufs}.values())

    def snap(fn):
        for b in bufs:
            b.reset()
        fn()
        torch.cuda.synchronize()
        return [b.t.clone() for b in bufs]
    single = snap(lambda: [L.launch(lib) for L in layers])
    run, variant, prefix = _group(lib, layers, dt)
    first, second = snap(run), snap(run)
    for i, (b, s, g1, g2) in enumerate(zip(bufs, single, first, second)):
        assert same_bits(g1, s), f"{what}: buffer {i} of the grouped launch differs from the single launches"
        assert same_bits(g2, g1), f"{what}: buffer {i} differs between two grouped launches"
    for i, L in enumerate(layers):
        L.check(f"{what}, layer {i}")
    for i, b in enumerate(bufs):
        b.check_untouched(f"{what}, buffer {i}")
    return variant, prefix


def _fwd_group(lib, dt, kind):
    if kind == "fwd_1x1_heads":        # Block35's three tower-entry 1x1 layers: one input, channel slices of one buffer, replicas
        x = _mk((2, 17, 17, 256), dt, seed=100)
        y, st = _Buf((2, 17, 17, 104), dt), _Acc(4, 128)
        return [_fwd_layer(lib, dt, (2, 17, 17, 256, 32, 1, 1, 1, 0, 0), 101 + 10 * i, y, c0=8 + 32 * i, x=x, stats=(st, 40 * i, 4 - i))
                for i in range(3)]
    if kind == "fwd_kxk":              # general gathers in one launch (ragged M = 162), ReLU / bias on members >= 1
        y1, y2, st = _Buf((2, 9, 9, 80), dt), _Buf((2, 9, 9, 64), dt), _Acc(2, 64)
        return [_fwd_layer(lib, dt, (2, 9, 9, 64, 32, 1, 7, 1, 0, 3), 110, y1, c0=0, stats=(st, 0, 2)),
                _fwd_layer(lib, dt, (2, 9, 9, 64, 32, 7, 1, 1, 3, 0), 120, y1, c0=40, bias=True, relu=1),
                _fwd_layer(lib, dt, (2, 9, 9, 48, 32, 3, 3, 1, 1, 1), 130, y2, c0=0, relu=1),
                _fwd_layer(lib, dt, (2, 19, 19, 48, 32, 3, 3, 2, 0, 0), 140, y2, c0=32, bias=True, stats=(st, 32, 1))]
    if kind == "fwd_up":               # the blocks' `up` layers: bias, residual, scale, with and without ReLU
        x = _mk((3, 8, 8, 96), dt, seed=150)
        y = _Buf((3, 8, 8, 200), dt)
        return [_fwd_layer(lib, dt, (3, 8, 8, 96, 64, 1, 1, 1, 0, 0), 151, y, c0=0, x=x, bias=True, resid=True, scale=0.17, relu=1),
                _fwd_layer(lib, dt, (3, 8, 8, 96, 64, 1, 1, 1, 0, 0), 161, y, c0=64, x=x, bias=True, resid=True, scale=0.1),
                _fwd_layer(lib, dt, (3, 8, 8, 96, 64, 1, 1, 1, 0, 0), 171, y, c0=136, x=x, bias=True, relu=1)]
    if kind == "fwd_64x64_ks2":        # in-launch split-K (tile pinned as the autotuner pins it)
        y, st = _Buf((3, 8, 8, 136), dt), _Acc(2, 136)
        return [_fwd_layer(lib, dt, (3, 8, 8, 128, 64, 1, 7, 1, 0, 3), 180, y, c0=0, stats=(st, 0, 2), tile=64064),
                _fwd_layer(lib, dt, (3, 8, 8, 128, 64, 7, 1, 1, 3, 0), 190, y, c0=72, bias=True, relu=1, tile=64064)]
    raise KeyError(kind)


def _dgrad_group(lib, dt, kind):
    if kind == "dgrad_8":              # eight layers, one of them a single workgroup: accumulate, fused BN reduction, stride 2
        a, b, c = _Buf((2, 9, 9, 112), dt), _Buf((2, 19, 19, 40), dt), _Buf((1, 3, 3, 32), dt)
        bn = _Acc(3, 96)
        return [_dgrad_layer(lib, dt, (2, 9, 9, 32, 48, 3, 3, 1, 1, 1), 200, a, c0=0),
                _dgrad_layer(lib, dt, (2, 9, 9, 32, 48, 3, 3, 1, 1, 1), 210, a, c0=32, accumulate=1),
                _dgrad_layer(lib, dt, (2, 9, 9, 24, 48, 3, 3, 1, 1, 1), 220, a, c0=64, bn=(bn, 0, 3, 1)),
                _dgrad_layer(lib, dt, (2, 9, 9, 16, 32, 1, 7, 1, 0, 3), 230, a, c0=96, bn=(bn, 32, 2, 0)),
                _dgrad_layer(lib, dt, (2, 19, 19, 32, 48, 3, 3, 2, 0, 0), 240, b, c0=0),
                _dgrad_layer(lib, dt, (2, 19, 19, 8, 32, 3, 3, 2, 0, 0), 250, b, c0=32, accumulate=1),
                _dgrad_layer(lib, dt, (2, 9, 9, 32, 48, 7, 1, 1, 3, 0), 260, _Buf((2, 9, 9, 32), dt), bn=(bn, 56, 1, 1)),
                _dgrad_layer(lib, dt, (1, 3, 3, 32, 32, 3, 3, 1, 1, 1), 270, c)]
    if kind == "dgrad_32x64_ks4":        # in-launch split-K, with a fused residual backward member
        a = _Buf((2, 8, 8, 208), dt)
        return [_dgrad_layer(lib, dt, (2, 8, 8, 64, 160, 1, 7, 1, 0, 3), 280, a, c0=0, tile=32064),
                _dgrad_layer(lib, dt, (2, 8, 8, 128, 128, 3, 3, 1, 1, 1), 290, a, c0=72, accumulate=1, tile=32064),
                _dgrad_layer(lib, dt, (2, 8, 8, 64, 160, 1, 7, 1, 0, 3), 295, _Buf((2, 8, 8, 80), dt), c0=8, tile=32064,    # single-source rb_*
                             rb=dict(prev=True, mask=True, acc=0, scale=0.17))]
    raise KeyError(kind)


GROUPS = {"fwd_1x1_heads": (32032, 3), "fwd_kxk": (32032, 4), "fwd_up": (32032, 3), "fwd_64x64_ks2": (2064064, 2),
          "dgrad_8": (32032, 8), "dgrad_32x64_ks4": (4032064, 3)}


@pytest.mark.parametrize("dt", [_lib.FN_BF16, _lib.FN_F16])
@pytest.mark.parametrize("kind", list(GROUPS))
def test_grouped_convolutions_match_single_launches(lib, kind, dt):
    """fn_conv2d_grouped (how Trainer.step runs same-level forward / data-gradient convolutions of one tile variant) == the
    members' own fn_conv2d_fwd / fn_conv2d_dgrad launches bit for bit -- outputs, BatchNorm statistics over replicas, fused
    BatchNorm-backward sums -- the same bits on a second launch, every element within the fp64 bound, neighbours untouched."""
    layers = _fwd_group(lib, dt, kind) if kind.startswith("fwd") else _dgrad_group(lib, dt, kind)
    variant, prefix = _check_group(lib, layers, dt, kind)
    assert (variant, len(layers)) == GROUPS[kind]
    if kind == "dgrad_8":
        assert min(b - a for a, b in zip(prefix, prefix[1:])) == 1          # a member with a single workgroup


def test_conv_group_build_rejects_mixed_members(lib):
    """Layers that cannot share a grouped launch are refused at build time (ValueError), never launched."""
    dt = _lib.FN_BF16

    def desc(geo, dtype=dt, **kw):
        d = conv_probe(conv_desc(*geo, dtype))
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    def build(descs, op):
        n = len(descs)
        variant = lib.fn_conv2d_variant(C.byref(descs[0]), op)
        return lib.fn_conv2d_group_build((_lib.ConvDesc * n)(*descs), n, op, variant, (C.c_uint8 * (lib.fn_conv2d_arg_bytes() * n))(),
                                         (C.c_int32 * (n + 1))(), C.byref(C.c_int32(0)))
    one, kxk = (2, 9, 9, 64, 32, 1, 1, 1, 0, 0), (2, 9, 9, 64, 32, 3, 3, 1, 1, 1)
    assert build([desc(one), desc(one)], 0) > 0 and build([desc(kxk), desc(kxk)], 1) > 0        # the well-formed groups build
    st = torch.zeros(256, dtype=torch.int64, device="cuda")
    norm = dict(nrm_stats=ptr(st), nrm_beta=ptr(st), nrm_count=162, nrm_eps=1e-3, nrm_sq_off=64)
    sib = dict(dy2=4096, w2=4096, Cout2=32, ld_y2=32)
    cases = {"mixed dtypes": ([desc(one), desc(one, _lib.FN_F16)], 0),
             "1x1 with general": ([desc(one), desc((2, 9, 9, 64, 32, 3, 1, 1, 1, 0))], 0),
             "normalise-on-load with plain": ([desc(one, **norm), desc(one)], 0),
             "another variant": ([desc(one), desc(one, tile_fwd=64064)], 0),
             "sibling sources": ([desc(one), desc(one, **sib)], 1),
             "halo kernel": ([desc(kxk), desc(kxk, tile_dgrad=HALO)], 1)}
    for what, (descs, op) in cases.items():
        with pytest.raises(ValueError):
            _lib.check(build(descs, op), what)


def _fuse_rb(lib, dt, d, out, c0, g, ag, K, seed, keep, prev=True, mask=True, acc=0, scale=0.17, positive=False, rb_bufs=None):
    """Sets fn_conv_desc.rb_* on data-gradient descriptor d (fp64 gradient g, |.| sums ag, K products) and returns the _Layer
    checking the contract of include/facenet_hip.h against fp64:
        total = rb_prev + g,  m = total * [rb_out > 0],  rb_dtrunk (+)= m,  rb_dup = rb_scale * m,  rb_dbias += sum_pixels rb_dup.
    dx (`out` at c0) must keep its bits.  rb_bufs: (dtrunk _Buf, dup _Buf, dbias _Acc, dbias offset) to share buffers; by default
    they get dx's geometry and channel offset."""
    N, H, W, Cin = d.N, d.H, d.W, d.Cin
    M = N * H * W
    shape = tuple(out.t.shape)
    dtr, dup, dbias, boff = rb_bufs or (_Buf(shape, dt), _Buf(shape, dt), _Acc(1, Cin), 0)
    p = _mk((N, H, W, Cin), dt, seed=seed + 5) if prev else None
    o = _mk((N, H, W, Cin), dt, seed=seed + 6) if mask else None
    if positive:
        o = o.abs() + 0.5
    base = _mk((N, H, W, Cin), dt, seed=seed + 7) if acc else None
    pb = _Buf(shape, dt)                                  # rb_prev / rb_out live in buffers of dx's geometry too
    ob = _Buf(shape, dt)
    if prev:
        pb.init[..., c0:c0 + Cin] = p
    if mask:
        ob.init[..., c0:c0 + Cin] = o
    pb.reset(); ob.reset()
    dtr.claim(c0, Cin, base)
    dup.claim(c0, Cin)
    dbias.claim(boff, Cin, 1, sq=False)
    d.rb_prev = ptr(pb.t, c0) if prev else None
    d.rb_out = ptr(ob.t, c0) if mask else None
    d.rb_dtrunk, d.rb_dup, d.rb_dbias, d.rb_scale, d.rb_accumulate = ptr(dtr.t, c0), ptr(dup.t, c0), ptr(dbias.t, boff), scale, acc
    keep += [pb, ob, p, o, base]
    tot, atot = (g + p.double().cpu(), ag + p.double().abs().cpu()) if prev else (g, ag)
    mk = (o.double().cpu() > 0).double() if mask else torch.ones_like(tot)
    m, am = tot * mk, atot * mk
    t_ref, t_abs = (m + base.double().cpu(), am + base.double().abs().cpu()) if acc else (m, am)
    Mv, e = m.reshape(M, Cin) * scale, abs(scale) * (gamma(K + 2) * am.reshape(M, Cin))
    te = e + 2.0 ** -24 * (Mv.abs() + e)                  # error of the fp32 terms rb_scale * m that rb_dbias sums

    def checks(what):
        got_t, got_u = dtr.t[..., c0:c0 + Cin], dup.t[..., c0:c0 + Cin]
        assert_elementwise(got_t, t_ref, t_abs, K + 3, dt, what + ": rb_dtrunk")
        assert_elementwise(got_u, scale * m, abs(scale) * am, K + 4, dt, what + ": rb_dup")
        off = mk == 0                                      # masked elements are exactly zero
        assert float(got_u.float().cpu()[off].abs().sum()) == 0, what + ": rb_dup not exactly 0 under the mask"
        if not acc:
            assert float(got_t.float().cpu()[off].abs().sum()) == 0, what + ": rb_dtrunk not exactly 0 under the mask"
        assert_acc_sums(dbias.t[0, boff:boff + Cin], Mv.sum(0), Mv.abs().sum(0), ACC_GRAD_BITS, _tiles(M), what + ": rb_dbias",
                        term_err=te.sum(0))
    L = _Layer(1, d, keep, [checks], [out, dtr, dup, dbias, pb, ob])
    L.rb = dict(prev=p, mask=o, acc=acc, scale=scale, dtr=dtr, dup=dup, dbias=dbias, boff=boff, c0=c0, M=M)
    return L


def _unfused(lib, dt, L):
    """The sequence the fusion replaces: the data gradient accumulated onto rb_prev, then fn_residual_bwd (dx contiguous)."""
    d, r = _lib.ConvDesc.from_buffer_copy(L.d), L.rb
    N, H, W, Cin = d.N, d.H, d.W, d.Cin
    dx = r["prev"].clone() if r["prev"] is not None else torch.zeros(N, H, W, Cin, dtype=lp_dtype(dt), device="cuda")
    d.rb_prev = d.rb_out = d.rb_dtrunk = d.rb_dup = d.rb_dbias = None
    d.dx, d.accumulate = ptr(dx), 1
    _lib.check(lib.fn_conv2d_dgrad(C.byref(d), stream()))
    dtr = r["dtr"].init.clone() if r["acc"] else torch.zeros_like(dx)
    dup = torch.zeros_like(dx)
    dbias = torch.zeros(Cin, dtype=torch.int64, device="cuda")
    mask = r["mask"]
    _lib.check(lib.fn_residual_bwd(ptr(dx), ptr(mask) if mask is not None else None, ptr(dtr), ptr(dup), ptr(dbias), r["M"], Cin,
                                   r["scale"], 1 if mask is not None else 0, r["acc"], dt, stream()))
    torch.cuda.synchronize()
    return dtr, dup, dbias


def _run_rb(lib, L, dt, what):
    """One fused launch from fresh buffers: the contract against fp64, dx untouched, rb_dbias the same bits on a second run, and
    within one rounding of dx of the unfused sequence (rb_dtrunk bit for bit when it is not accumulated)."""
    bufs = list({id(b): b for b in L.bufs}.values())
    runs = []
    for _ in range(2):
        for b in bufs:
            b.reset()
        L.launch(lib)
        torch.cuda.synchronize()
        runs.append([b.t.clone() for b in bufs])
    for i, (a, b) in enumerate(zip(*runs)):
        assert same_bits(a, b), f"{what}: buffer {i} differs between two runs"
    L.check(what)
    for i, b in enumerate(bufs):
        b.check_untouched(f"{what}, buffer {i}")          # dx (buffer 0) is not written at all
    r = L.rb
    c0, Cin = r["c0"], L.d.Cin
    if L.d.ld_x != Cin:
        return
    dtr_u, dup_u, dbias_u = _unfused(lib, dt, L)
    got_t, got_u = r["dtr"].t[..., c0:c0 + Cin], r["dup"].t[..., c0:c0 + Cin]
    u, s = U_LP[dt], abs(r["scale"])
    tu = dtr_u.double().cpu() - (r["dtr"].init.double().cpu() if r["acc"] else 0)      # the masked gradient, rounded once
    if not r["acc"]:
        assert same_bits(got_t, dtr_u), f"{what}: rb_dtrunk differs from the unfused sequence"
    else:
        assert bool(((got_t.double().cpu() - dtr_u.double().cpu()).abs() <= 2.01 * u * (tu.abs() + dtr_u.double().cpu().abs()) + 1e-7).all()), what
    du = dup_u.double().cpu().abs()                        # |rb_scale * m| within (1 + u)^2: one rounding of dx, one of the product
    assert bool(((got_u.double().cpu() - dup_u.double().cpu()).abs() <= 3.1 * u * du + 1e-7).all()), what + ": rb_dup vs unfused"
    db, dbu = r["dbias"].t[0, r["boff"]:r["boff"] + Cin].double().cpu(), dbias_u.double().cpu()
    tol = (1.1 * u + 2 * gamma(r["M"])) * du.reshape(-1, Cin).sum(0) + 2 * r["M"] * 2.0 ** -ACC_GRAD_BITS
    assert bool(((db - dbu).abs() * 2.0 ** -ACC_GRAD_BITS <= tol).all()), what + ": rb_dbias vs unfused"


RB_BLOCKS = {"block35": (2, 17, 17, 256, [32, 32, 32], 0.17), "block17": (2, 8, 8, 896, [128, 128], 0.10),
             "block8": (5, 3, 3, 1792, [192, 192], 0.2)}      # block8: N*H*W = 45 rows, ragged in every tile
RB_CASES = [(b, n) for b, v in RB_BLOCKS.items() for n in range(1, len(v[4]) + 1)]


@pytest.mark.parametrize("dt", [_lib.FN_BF16, _lib.FN_F16])
@pytest.mark.parametrize("tile", [0, 128064, 64064, 32032, 32128])
@pytest.mark.parametrize("block,nsrc", RB_CASES)
def test_dgrad_fused_residual_backward_production_flags(lib, block, nsrc, tile, dt):
    """The residual backward in the epilogue of the merged sibling data gradient (engine._fuse_residual) with the flags
    production sets (rb_prev, rb_out, rb_accumulate = 0): 1-3 sources at the widths of Block35 / Block17 / Block8."""
    N, H, W, Cin, couts, scale = RB_BLOCKS[block]
    L = _dgrad_layer(lib, dt, (N, H, W, Cin, couts[0], 1, 1, 1, 0, 0), 300, _Buf((N, H, W, Cin), dt), tile=tile, siblings=couts[1:nsrc],
                     rb=dict(prev=True, mask=True, acc=0, scale=scale))
    _run_rb(lib, L, dt, f"{block} x{nsrc} tile {tile}")


@pytest.mark.parametrize("dt", [_lib.FN_BF16, _lib.FN_F16])
def test_dgrad_fused_residual_backward_all_flags(lib, dt):
    """Every combination of rb_out (NULL: no activation), rb_prev (NULL: nothing carried) and rb_accumulate (1 leaves the
    dedicated epilogue path for the generic one), on a two-source Block17 data gradient; with rb_prev = NULL, rb_out > 0
    everywhere and no accumulation, rb_dtrunk is the plain data gradient of the same tile bit for bit."""
    geo, sib = (2, 8, 8, 896, 128, 1, 1, 1, 0, 0), [128]
    for prev in (True, False):
        for mask in (True, False):
            for acc in (0, 1):
                L = _dgrad_layer(lib, dt, geo, 400, _Buf((2, 8, 8, 896), dt), siblings=sib, rb=dict(prev=prev, mask=mask, acc=acc, scale=0.1))
                _run_rb(lib, L, dt, f"prev {prev} mask {mask} acc {acc}")
    L = _dgrad_layer(lib, dt, geo, 400, _Buf((2, 8, 8, 896), dt), siblings=sib, rb=dict(prev=False, mask=True, acc=0, scale=0.1, positive=True))
    _run_rb(lib, L, dt, "rb_out > 0")
    plain = _lib.ConvDesc.from_buffer_copy(L.d)
    plain.rb_prev = plain.rb_out = plain.rb_dtrunk = plain.rb_dup = plain.rb_dbias = None
    dx = torch.full((2, 8, 8, 896), float("nan"), dtype=lp_dtype(dt), device="cuda")
    plain.dx = ptr(dx)
    _lib.check(lib.fn_conv2d_dgrad(C.byref(plain), stream()))
    torch.cuda.synchronize()
    assert same_bits(dx, L.rb["dtr"].t)


@pytest.mark.parametrize("dt", [_lib.FN_BF16, _lib.FN_F16])
@pytest.mark.parametrize("layer", ["stride2", "halo"])
def test_dgrad_fused_residual_backward_single_source_layers(lib, layer, dt):
    """rb_* on the single-source data gradients the ABI allows besides the 1x1 siblings: a 3x3 stride-2 layer (parity classes,
    row table) and a 3x3 layer on the halo-tile kernel; dx a channel slice of a wider buffer."""
    geo, tile = {"stride2": ((2, 17, 17, 64, 64, 3, 3, 2, 0, 0), 0), "halo": ((1, 37, 37, 32, 32, 3, 3, 1, 1, 1), HALO)}[layer]
    for acc in (0, 1):
        N, H, W, Cin = geo[:4]
        L = _dgrad_layer(lib, dt, geo, 500, _Buf((N, H, W, Cin + 16), dt), c0=8, tile=tile, rb=dict(prev=True, mask=True, acc=acc, scale=0.2))
        assert (_lib.variant_is_halo(lib.fn_conv2d_variant(C.byref(L.d), 1))) == (layer == "halo")
        _run_rb(lib, L, dt, f"{layer} acc {acc}")
        L = _dgrad_layer(lib, dt, geo, 500, _Buf((N, H, W, Cin), dt), tile=tile, rb=dict(prev=True, mask=True, acc=acc, scale=0.2))
        _run_rb(lib, L, dt, f"{layer} acc {acc}, contiguous")


SPLITK = [  # (BM, BN, KS), the layer: 3x3 'same' with Cin == Cout on 9x9 maps (M = 162: ragged row tiles), forward == dgrad GEMM shape
    (32, 128, 2, 128), (32, 64, 2, 64), (32, 64, 4, 128), (32, 32, 2, 64), (32, 32, 4, 128), (64, 64, 2, 64), (64, 32, 2, 64)]


@pytest.mark.parametrize("dt", [_lib.FN_BF16, _lib.FN_F16])
@pytest.mark.parametrize("bm,bn,ks,c", SPLITK)
def test_conv_split_k_variants(lib, bm, bn, ks, c, dt):
    """Every in-launch split-K variant the library heuristic picks for a pinned tile (the autotuner pins tiles; the ks choice is
    the heuristic's): fn_conv2d_variant must name exactly this variant -- a heuristic change cannot drop the coverage silently --
    then forward + BatchNorm statistics and the data gradient + fused BatchNorm reduction, element by element against fp64.
    (64x64 / 64x32 four-way split-K are reachable only through FN_CONV_KS64_4, read once per process: not covered here.)"""
    geo, tile = (2, 9, 9, c, c, 3, 3, 1, 1, 1), bm * 1000 + bn
    st, bn_acc = _Acc(2, c), _Acc(3, c)
    f = _fwd_layer(lib, dt, geo, 600, _Buf((2, 9, 9, c), dt), stats=(st, 0, 2), tile=tile)
    g = _dgrad_layer(lib, dt, geo, 610, _Buf((2, 9, 9, c), dt), bn=(bn_acc, 0, 3, 1), tile=tile)
    for L in (f, g):
        assert lib.fn_conv2d_variant(C.byref(L.d), L.op) == ks * 1000000 + tile
        for b in L.bufs:
            b.reset()
        L.launch(lib)
        torch.cuda.synchronize()
        L.check(f"{bm}x{bn} ks {ks} op {L.op}")
        for b in L.bufs:
            b.check_untouched(f"{bm}x{bn} ks {ks} op {L.op}")


# ---- element-wise bounds: single launches, the halo-tile kernel, every pinnable tile, sibling sources, normalise-on-load, nrm_z ----
# The launches the rel_err tests above run, held element by element: outputs start as NaN inside wider bit-patterned buffers
# (channels [8, 8 + C)), BatchNorm statistics go to 4 replicas at a non-zero column offset, and every test asserts the variant
# fn_conv2d_variant names for its launch.  (Weight gradients: tests/test_gpu_conv_wgrad.py.)

# fn_conv2d_variant(d, 0) / (d, 1) of CASES under the library heuristic (HALO_CASES: with the halo-tile kernel requested)
CASE_VARIANTS = [(32032, 32032), (32032, 2032032), (32032, 32032), (2032032, 4032032), (32032, 32032), (32032, 32032), (4032032, 2032032),
                 (2032032, 2032032), (2032032, 2032032), (2032032, 2032032), (2032032, 2032032), (32032, 4032032), (4032032, 32032),
                 (9000064, 9000032), (9000064, 9000032), (9000032, 9000032), (9000032, 9000064),
                 (4032032, 4032032), (32032, 32032), (32032, 2032032), (32032, 32032), (32032, 32032), (4032032, 32032),      # v2: Mixed_5a .. Mixed_6a
                 (4032032, 32032), (2032032, 4032032), (4032032, 4032032), (32032, 2032032), (4032032, 4032032), (4032032, 4032032),   # block17, Mixed_7a
                 (4032032, 32032), (2032032, 2032032), (2032032, 2032032), (32032, 4032032), (2032032, 32032), (4032032, 32032),      # block8 .. Bottleneck
                 (9000032, 9000032)]                                                                                                   # halo at 299, unrequested
NINE_TILES = [128128, 128064, 128032, 64128, 64064, 64032, 32128, 32064, 32032]


def _launch_checked(lib, L, what):
    for b in L.bufs:
        b.reset()
    L.launch(lib)
    torch.cuda.synchronize()
    L.check(what)
    for b in L.bufs:
        b.check_untouched(what)


@pytest.mark.parametrize("dt", [_lib.FN_BF16, _lib.FN_F16])
@pytest.mark.parametrize("case", CASES)
def test_conv_single_launches_elementwise(lib, case, dt):
    """Every layer of CASES as a single launch against fp64, element by element: forward with BatchNorm statistics over four
    replicas, the data gradient plain and accumulated onto a base; the four HALO_CASES on conv_halo_kernel (tile 9000000), where
    one wrong border pixel of one tile fails.  The Block35 3x3 layer of the 299-pixel geometry (1, 35, 35, 32, 48) asks for no
    tile: CASE_VARIANTS holds the library to choosing the halo-tile kernel for it, forward and data gradient."""
    N, H, W, Cin, Cout, kh, kw, s, ph, pw, OH, OW = _geo(case)
    tile = HALO if case in HALO_CASES else 0
    want = CASE_VARIANTS[CASES.index(case)]
    f = _fwd_layer(lib, dt, case, 800, _Buf((N, OH, OW, Cout + 16), dt), c0=8, stats=(_Acc(4, Cout + 8), 8, 4), tile=tile)
    g0 = _dgrad_layer(lib, dt, case, 810, _Buf((N, H, W, Cin + 16), dt), c0=8, tile=tile)
    g1 = _dgrad_layer(lib, dt, case, 810, _Buf((N, H, W, Cin + 16), dt), c0=8, accumulate=1, tile=tile)
    for L, what in ((f, "forward"), (g0, "dgrad"), (g1, "dgrad, accumulate")):
        assert lib.fn_conv2d_variant(C.byref(L.d), L.op) == want[L.op]
        _launch_checked(lib, L, f"{case} {what}")


@pytest.mark.parametrize("tile", NINE_TILES)
@pytest.mark.parametrize("case", TILE_CASES)
def test_conv_explicit_tiles_elementwise(lib, case, tile):
    """test_conv_explicit_tiles element by element: every tile a caller may pin, forward with BatchNorm statistics and data
    gradient, against one fp64 reference per layer."""
    dt = _lib.FN_BF16
    N, H, W, Cin, Cout, kh, kw, s, ph, pw, OH, OW = _geo(case)
    f = _fwd_layer(lib, dt, case, 820, _Buf((N, OH, OW, Cout + 16), dt), c0=8, stats=(_Acc(4, Cout + 8), 8, 4), tile=tile)
    g = _dgrad_layer(lib, dt, case, 830, _Buf((N, H, W, Cin + 16), dt), c0=8, tile=tile)
    for L in (f, g):
        assert _lib.variant_tile(lib.fn_conv2d_variant(C.byref(L.d), L.op)) == tile          # (+ KS * 1000000: in-launch split-K)
        _launch_checked(lib, L, f"{case} tile {tile} op {L.op}")


@pytest.mark.parametrize("tile", [0, 128064, 64064, 32032, 32128])
@pytest.mark.parametrize("nsrc", [2, 3])
@pytest.mark.parametrize("dt", [_lib.FN_BF16, _lib.FN_F16])
def test_dgrad_sibling_sources_elementwise(lib, dt, nsrc, tile):
    """The multi-source data gradient of test_dgrad_sibling_sources_equal_the_sum_of_single_dgrads (dY slices of wider buffers,
    ld_y2 / ld_y3 > Cout, K tails that are no multiples of the 64-wide k tile) element by element against the fp64 sum of the
    per-layer gradients, plain and accumulated."""
    N, H, W, Cin = 3, 9, 9, 256
    couts, lds = [32, 40, 96][:nsrc], [96, 40, 160][:nsrc]
    for acc in (0, 1):
        L = _dgrad_layer(lib, dt, (N, H, W, Cin, couts[0], 1, 1, 1, 0, 0), 840, _Buf((N, H, W, Cin + 16), dt), c0=8, accumulate=acc, tile=tile,
                         siblings=couts[1:], lds=lds)
        assert lib.fn_conv2d_variant(C.byref(L.d), 1) == (tile or 32032)                      # sibling launches never split K
        _launch_checked(lib, L, f"{nsrc} sources, tile {tile}, accumulate {acc}")


def _norm_fwd(lib, dt, case, seed, tile=0, z_out=None):
    """A normalise-on-load forward launch (x: the raw slice of tests.test_gpu_conv_wgrad._bn_operand) into a NaN-prefilled slice
    of a wider buffer; the reference is conv_fp64 of the tensor fn_bn_relu_train_fwd writes from the same statistics."""
    from tests.test_gpu_conv_wgrad import _bn_operand
    N, H, W, Cin, Cout, kh, kw, s, ph, pw, OH, OW = _geo(case)
    raw, z, set_norm, keep = _bn_operand(lib, case, dt, seed)
    w = _mk((Cout, kh, kw, Cin), dt, 0.1, seed=seed + 1)
    out = _Buf((N, OH, OW, Cout + 16), dt)
    out.claim(8, Cout)
    d = conv_desc(N, H, W, Cin, Cout, kh, kw, s, ph, pw, dt, ld_x=Cin + 16, ld_y=Cout + 16)
    d.w, d.y, d.tile_fwd = ptr(w), ptr(out.t, 8), tile
    set_norm(d)
    if z_out is not None:
        d.nrm_z = ptr(z_out.t, 8)
    zs = z[..., 8:8 + Cin]
    ref, aref = _memo(("norm fwd", case, dt, seed), lambda: conv_fp64(zs, w, s, ph, pw))
    check = lambda what: assert_elementwise(out.t[..., 8:8 + Cout], ref, aref, kh * kw * Cin + 3, dt, what + ": y")
    return _Layer(0, d, [raw, z, w, keep], [check], [out] + ([z_out] if z_out is not None else [])), zs


@pytest.mark.parametrize("dt", [_lib.FN_BF16, _lib.FN_F16])
@pytest.mark.parametrize("case", NORM_CASES)
def test_conv_normalise_on_load_forward_elementwise(lib, case, dt):
    """The forward half of test_conv_normalise_on_load_equals_materialised_bn against fp64: y from the RAW tensor and its
    statistics == the convolution of the materialised activation, element by element, zero padding included."""
    L, zs = _norm_fwd(lib, dt, case, 850)
    assert lib.fn_conv2d_variant(C.byref(L.d), 0) == 32032                                    # normalise-on-load never splits K
    _launch_checked(lib, L, f"{case} normalise-on-load")


NRMZ_LAYERS = [(3, 9, 9, 64, 160, 1, 1, 1, 0, 0), (2, 9, 9, 64, 160, 3, 3, 1, 1, 1)]      # M = 243 / 162: ragged in every row tile


@pytest.mark.parametrize("dt", [_lib.FN_BF16, _lib.FN_F16])
@pytest.mark.parametrize("tile", [32032, 128064])
@pytest.mark.parametrize("case", NRMZ_LAYERS)
def test_conv_nrm_z_side_write(lib, case, tile, dt):
    """fn_conv_desc.nrm_z: the activated tensor the lazy BatchNorm plan lets its single reader write.  Cout = 160 spans five /
    three column tiles (only the first tile's workgroups write), x and nrm_z are slices of wider buffers.  The contract is
    bit-equality: nrm_z, NaN-prefilled, afterwards holds exactly what fn_bn_relu_train_fwd writes from the same statistics (the
    same fma, ReLU and rounding), its neighbour bytes untouched; y is within the fp64 bound and bit-identical to the launch
    without nrm_z."""
    N, H, W, Cin, Cout, kh, kw, s, ph, pw, OH, OW = _geo(case)
    zb = _Buf((N, H, W, Cin + 16), dt)
    zb.claim(8, Cin)
    plain, zs = _norm_fwd(lib, dt, case, 860, tile=tile)
    side, _ = _norm_fwd(lib, dt, case, 860, tile=tile, z_out=zb)
    for L in (plain, side):
        assert lib.fn_conv2d_variant(C.byref(L.d), 0) == tile
        _launch_checked(lib, L, f"{case} tile {tile} nrm_z {L is side}")
    assert same_bits(side.bufs[0].t, plain.bufs[0].t), "y differs with nrm_z"
    assert same_bits(zb.t[..., 8:8 + Cin], zs), "nrm_z differs from fn_bn_relu_train_fwd's output"
    first = zb.t.clone()
    side.launch(lib)                                        # again onto the written tensor: the same bits
    torch.cuda.synchronize()
    assert same_bits(zb.t, first)


def test_conv_nrm_z_rejections(lib):
    """nrm_z needs stride 1 and an output map of the input's size, and it needs nrm_stats: refused before any launch."""
    dt = _lib.FN_BF16
    t = torch.zeros(2 * 9 * 9 * 160, dtype=lp_dtype(dt), device="cuda")
    st = torch.zeros(256, dtype=torch.int64, device="cuda")
    for geo, norm in (((2, 9, 9, 64, 160, 3, 3, 2, 1, 1), True), ((2, 9, 9, 64, 160, 3, 3, 1, 0, 0), True), ((2, 9, 9, 64, 160, 3, 3, 1, 1, 1), False)):
        d = conv_desc(*geo, dt)
        d.x = d.w = d.y = d.nrm_z = ptr(t)
        if norm:
            d.nrm_stats, d.nrm_beta, d.nrm_count, d.nrm_eps, d.nrm_sq_off = ptr(st), ptr(st), 162, 1e-3, 64
        with pytest.raises(ValueError):
            _lib.check(lib.fn_conv2d_fwd(C.byref(d), stream()))
        d.nrm_z = None
        if norm:                                            # the same descriptor without nrm_z is a valid launch
            assert lib.fn_conv2d_variant(C.byref(d), 0) > 0
