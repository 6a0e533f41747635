"""The kernels of csrc/elementwise.hip at their edge shapes, element by element against fp64 (bounds and references:
tests/elementwise_oracle.py; the bounds themselves are checked in tests/test_elementwise_refs_host.py).  Every case names the
branch it is for.  Where the kernel's arithmetic is one rounding of an exactly representable fp32 expression the comparison is
bit for bit; every output that is a slice of a wider buffer is pre-filled with a bit pattern and the bytes outside the slice are
compared afterwards."""
import numpy as np
import pytest
import torch

from facenet_amd import _lib
from tests import elementwise_oracle as eo
from tests import irv2_oracle as ro
from tests.util import (ACC_GRAD_BITS, assert_acc_sums, assert_elementwise, bitpattern, lp_dtype, ptr, same_bits, stream)

pytestmark = pytest.mark.gpu
BF, HF = _lib.FN_BF16, _lib.FN_F16
DTS = [BF, HF]
GRID_CAP = 4096 * 256             # grid_for: work items beyond this take a second trip of the grid-stride loop


def _lp_rand(shape, dt, seed, scale=1.0, shift=0.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale + shift).to(lp_dtype(dt))


def _in_slice(buf, c0, C, data):
    """A [M, ld] device buffer of bit pattern with `data` in columns c0 .. c0 + C."""
    buf[..., c0:c0 + C] = data.to(buf.device)
    return buf


def _outside_untouched(buf, before, c0, C):
    mask = torch.ones(buf.shape[-1], dtype=torch.bool)
    mask[c0:c0 + C] = False
    return same_bits(buf[..., mask], before[..., mask])


# ---- BatchNorm + ReLU, training -------------------------------------------------------------------------------------------
BN_CASES = eo.bn_cases()


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("case", BN_CASES, ids=[c[0] for c in BN_CASES])
def test_bn_relu_train_edges(lib, case, dt):
    """Stripe widths 1..8, short / ragged row chunks, rows_per_block = 35, 1 / 3 / 7 replicas with a stride and junk between the
    columns, reduced 0 / 1, relu 0 / 1, moving statistics present / NULL, slices with ld_y != ld_z.  Stage 1: saved scale / shift and
    the moving statistics against fp64 from the exact sums.  Stage 2: z, dz, the backward sums and dbeta against fp64 from the scale
    and shift the kernel saved."""
    name, M, C, c0, ld_y, ld_z, reps, relu, moving, reduced, far = case
    seed = sum(name.encode()) % 1000
    y, dz, beta, S1, S2 = eo.bn_inputs(dt, M, C, seed, far)
    sq_off, stride = C + 8, 2 * C + 24
    stats = eo.acc_buffer(eo.split_replicas(S1, reps, 1), eo.split_replicas(S2, reps, 2), C, sq_off, stride).cuda()
    ybuf = _in_slice(bitpattern((M, ld_y), dt), c0, C, y)
    zbuf = bitpattern((M, ld_z), dt)
    z_before = zbuf.clone()
    beta_d = beta.cuda()
    sc, sh = torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")
    mm0, mv0 = torch.linspace(-1, 1, C), torch.linspace(0.5, 2, C)
    mm, mv = mm0.cuda(), mv0.cuda()
    _lib.check(lib.fn_bn_relu_train_fwd(ptr(ybuf, c0), ld_y, ptr(zbuf, c0), ld_z, M, C, ptr(stats), sq_off, reps, stride, ptr(beta_d), ptr(sc),
                                        ptr(sh), ptr(mm) if moving else None, ptr(mv) if moving else None, 0.99, 1e-3, relu, dt, stream()))
    torch.cuda.synchronize()
    ref = eo.bn_affine_ref(S1, S2, M, 1e-3, beta)
    eo.check_bound(sc, ref["scale"], ref["e_scale"], f"{name} save_scale")
    eo.check_bound(sh, ref["shift"], ref["e_shift"], f"{name} save_shift")
    if moving:
        want, bound = eo.bn_moving_ref(mm0, ref["mean"], ref["e_mean"], 0.99)
        eo.check_bound(mm, want, bound, f"{name} moving_mean")
        want, bound = eo.bn_moving_ref(mv0, ref["var"], ref["e_var"], 0.99)
        eo.check_bound(mv, want, bound, f"{name} moving_var")
    else:
        assert torch.equal(mm.cpu(), mm0) and torch.equal(mv.cpu(), mv0)
    sc_c, sh_c = sc.cpu(), sh.cpu()
    assert eo.bn_zero_margin(y, sc_c, sh_c) == 0, "an element whose ReLU decision is ambiguous"        # share of excluded elements: 0
    zr, za, k = eo.bn_fwd_ref(y, sc_c, sh_c, relu)
    assert_elementwise(zbuf[:, c0:c0 + C], zr, za, k, dt, f"{name} z")
    assert _outside_untouched(zbuf, z_before, c0, C), "bn_fwd wrote outside its channel slice"
    # backward
    dbuf = _in_slice(bitpattern((M, ld_z), dt), c0, C, dz)
    d_before = dbuf.clone()
    dbeta0 = torch.linspace(-2, 2, C)
    dbeta = dbeta0.cuda()
    rows, tiles = eo.reduce_chain(M, C)
    if reduced:     # the test supplies the sums a dgrad epilogue would have left, spread unevenly over the replicas
        A1, A2 = eo.bn_sums_f32(dz, y, sc_c, sh_c, beta, relu, M, C)
        acc = eo.acc_buffer(eo.split_replicas(A1, reps, 3), eo.split_replicas(A2, reps, 4), C, sq_off, stride).cuda()
    else:           # the kernel reduces into replica 0; the other replicas hold parts that cancel exactly
        zero = torch.zeros(C, dtype=torch.int64)
        p1, p2 = eo.split_replicas(zero, reps, 3), eo.split_replicas(zero, reps, 4)
        if reps > 1:
            p1[1] += p1[0]; p1[0] = 0
            p2[1] += p2[0]; p2[0] = 0
        acc = eo.acc_buffer(p1, p2, C, sq_off, stride).cuda()
    _lib.check(lib.fn_bn_relu_train_bwd(ptr(dbuf, c0), ld_z, ptr(ybuf, c0), ld_y, M, C, ptr(beta_d), ptr(sc), ptr(sh), ptr(dbeta), ptr(acc), sq_off,
                                        reps, stride, reduced, relu, dt, stream()))
    torch.cuda.synchronize()
    accv = acc.cpu().view(reps, stride)
    A1, A2 = accv[:, :C].sum(0), accv[:, sq_off:sq_off + C].sum(0)
    junk = torch.ones(stride, dtype=torch.bool)
    junk[:C] = False
    junk[sq_off:sq_off + C] = False
    assert bool((accv[:, junk] == 0x5A5A5A5A5A5A).all()), "the reduction wrote outside its columns"
    if not reduced:
        r1, a1, r2, a2, te2 = eo.bn_sums_ref(dz, y, sc_c, sh_c, beta, relu)
        assert_acc_sums(A1, r1, a1, ACC_GRAD_BITS, tiles, f"{name} sum dyh", rows=rows)
        assert_acc_sums(A2, r2, a2, ACC_GRAD_BITS, tiles, f"{name} sum dyh xhat", term_err=te2, rows=rows)
    dr, da, kb = eo.bn_bwd_ref(dz, y, sc_c, sh_c, beta, A1, A2, M, relu)
    assert_elementwise(dbuf[:, c0:c0 + C], dr, da, kb, dt, f"{name} dz")
    assert _outside_untouched(dbuf, d_before, c0, C), "bn_bwd wrote outside its channel slice"
    s1 = A1.double() * 2.0 ** -ACC_GRAD_BITS                 # dbeta = fl(dbeta + fl(S1)): 2 roundings
    assert_elementwise(dbeta, dbeta0.double() + s1, dbeta0.double().abs() + s1.abs(), 2, dt, f"{name} dbeta", out_f32=True)


def test_bn_finalize_matches_the_forward_kernel_bits(lib):
    """fn_bn_finalize and fn_bn_relu_train_fwd publish the same scale / shift bits from replicated sums (7 replicas: not a
    multiple of the 4 thread groups that add them)."""
    M, C, reps = 300, 104, 7
    y, _, beta, S1, S2 = eo.bn_inputs(BF, M, C, 5)
    sq_off, stride = C + 8, 2 * C + 24
    stats = eo.acc_buffer(eo.split_replicas(S1, reps, 1), eo.split_replicas(S2, reps, 2), C, sq_off, stride).cuda()
    beta_d = beta.cuda()
    sc, sh, sc2, sh2 = (torch.zeros(C, device="cuda") for _ in range(4))
    ybuf, zbuf = y.cuda(), torch.zeros(M, C, dtype=torch.bfloat16, device="cuda")
    _lib.check(lib.fn_bn_relu_train_fwd(ptr(ybuf), C, ptr(zbuf), C, M, C, ptr(stats), sq_off, reps, stride, ptr(beta_d), ptr(sc), ptr(sh), None, None,
                                        0.99, 1e-3, 1, BF, stream()))
    rp = torch.full((C,), reps, dtype=torch.int32, device="cuda")
    cnt = torch.full((C,), M, dtype=torch.int32, device="cuda")
    _lib.check(lib.fn_bn_finalize(ptr(stats), sq_off, stride, ptr(rp), ptr(cnt), ptr(beta_d), ptr(sc2), ptr(sh2), None, None, 0.99, 1e-3, C, stream()))
    torch.cuda.synchronize()
    assert torch.equal(sc, sc2) and torch.equal(sh, sh2)
    ref = eo.bn_affine_ref(S1, S2, M, 1e-3, beta)
    eo.check_bound(sc2, ref["scale"], ref["e_scale"], "finalize scale")
    eo.check_bound(sh2, ref["shift"], ref["e_shift"], "finalize shift")


def test_bn_bwd_rejects_row_strides_below_the_channel_count(lib):
    """Decided on the host before any launch, like the forward's check."""
    t = torch.zeros(64, 64, dtype=torch.bfloat16, device="cuda")
    f = torch.zeros(64, device="cuda")
    acc = torch.zeros(128, dtype=torch.int64, device="cuda")
    for ld_d, ld_y in ((32, 64), (64, 32)):
        with pytest.raises(ValueError, match="must be >= C"):
            _lib.check(lib.fn_bn_relu_train_bwd(ptr(t), ld_d, ptr(t), ld_y, 8, 64, ptr(f), ptr(f), ptr(f), ptr(f), ptr(acc), 64, 1, 0, 0, 1, BF, stream()))
    with pytest.raises(ValueError):
        _lib.check(lib.fn_bn_relu_train_fwd(ptr(t), 32, ptr(t), 64, 8, 64, ptr(acc), 64, 1, 0, ptr(f), ptr(f), ptr(f), None, None, 0.99, 1e-3, 1, BF, stream()))


# ---- residual backward ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("relu", [1, 0])
@pytest.mark.parametrize("M", [5, 300])                     # M < 32: one short row chunk
@pytest.mark.parametrize("C", [8, 24, 256, 2080])           # 2080 = 32 stripes + a last stripe of 4 groups (Inception-ResNet-v2)
def test_residual_bwd_edges(lib, C, M, relu, accumulate, dt):
    """dtrunk = round(g (+ prev)) and dup = round(fp32(scale g)) bit for bit, dbias by the fixed-point bound, the same bits run to
    run; relu = 0 passes out = NULL."""
    out = _lp_rand((M, C), dt, 9, 1.0).clamp(min=0)
    dout = _lp_rand((M, C), dt, 10)
    prev = _lp_rand((M, C), dt, 11)
    want_trunk, want_up, ref, absref = eo.residual_ref(dout, out, prev, 0.17, relu, accumulate)
    rows, tiles = eo.reduce_chain(M, C)
    first = None
    for _ in range(2):
        dtrunk, dup = prev.cuda().clone(), bitpattern((M, C), dt)
        dbias = torch.zeros(C, dtype=torch.int64, device="cuda")
        out_d, dout_d = out.cuda(), dout.cuda()
        _lib.check(lib.fn_residual_bwd(ptr(dout_d), ptr(out_d) if relu else None, ptr(dtrunk), ptr(dup), ptr(dbias), M, C, 0.17, relu, accumulate,
                                       dt, stream()))
        torch.cuda.synchronize()
        assert same_bits(dtrunk, want_trunk) and same_bits(dup, want_up)
        # terms fl(scale g) carry u |scale g| each; chain: the thread's rows, then 32 partial sums
        assert_acc_sums(dbias, ref, absref, ACC_GRAD_BITS, tiles, "dbias", term_err=eo.U * absref, rows=eo.cdiv(eo.reduce_rows_per_block(M, C), 32) + 32)
        if first is None:
            first = dbias.clone()
        assert torch.equal(dbias, first)


# ---- max-pool 3x3 / 2 ---------------------------------------------------------------------------------------------------
def _maxpool_case(lib, dt, N, H, W, C, c0, ld_x, ld_y, x):
    OH, OW = (H - 3) // 2 + 1, (W - 3) // 2 + 1
    xbuf = _in_slice(bitpattern((N, H, W, ld_x), dt), c0, C, x)
    ybuf = bitpattern((N, OH, OW, ld_y), dt)
    y_before = ybuf.clone()
    amax = torch.full((N, OH, OW, C), 255, dtype=torch.uint8, device="cuda")
    _lib.check(lib.fn_maxpool3x3s2_fwd(ptr(xbuf, c0), ld_x, ptr(ybuf, c0), ld_y, N, H, W, C, ptr(amax), dt, stream()))
    torch.cuda.synchronize()
    want_y, want_am = eo.maxpool_ref(x)
    assert same_bits(ybuf[..., c0:c0 + C], want_y), "max-pool forward differs from the first-maximum reference"
    assert torch.equal(amax.cpu(), want_am), "argmax bytes differ"
    assert _outside_untouched(ybuf, y_before, c0, C)
    dy = _lp_rand((N, OH, OW, C), dt, 6)
    dybuf = _in_slice(bitpattern((N, OH, OW, ld_y), dt), c0, C, dy)
    ref, absref = eo.maxpool_bwd_ref(dy, want_am, H, W)
    prev = _lp_rand((N, H, W, C), dt, 7)
    covered = torch.zeros(H, W, dtype=torch.bool)
    covered[:2 * OH + 1, :2 * OW + 1] = True
    for accumulate in (0, 1):
        res = []
        for use_amax in (False, True):
            dxbuf = _in_slice(bitpattern((N, H, W, ld_x), dt), c0, C, prev)
            before = dxbuf.clone()
            _lib.check(lib.fn_maxpool3x3s2_bwd(None if use_amax else ptr(xbuf, c0), ld_x, ptr(dybuf, c0), ld_y, ptr(dxbuf, c0), ld_x, N, H, W, C,
                                               ptr(amax) if use_amax else None, accumulate, dt, stream()))
            torch.cuda.synchronize()
            assert _outside_untouched(dxbuf, before, c0, C)
            res.append(dxbuf[..., c0:c0 + C].cpu())
        assert same_bits(res[0], res[1]), "recomputation and argmax forms of the max-pool backward differ"
        p = prev.double() if accumulate else torch.zeros_like(ref)
        assert_elementwise(res[0], ref + p, absref + p.abs(), 5, dt, f"maxpool dx accumulate={accumulate}")      # <= 4 addends + prev
        # rows / columns no window covers: exactly 0, or the previous value
        want = prev if accumulate else torch.zeros_like(prev)
        assert same_bits(res[0][:, ~covered], want[:, ~covered])


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("H,W", [(3, 3), (4, 5), (8, 8), (17, 17), (35, 34)])
@pytest.mark.parametrize("C,c0,ld_x,ld_y", [(8, 0, 8, 8), (40, 8, 64, 48)])
def test_maxpool_edges(lib, H, W, C, c0, ld_x, ld_y, dt):
    """One window (3 x 3), even H / W (last row / column in no window), H != W, a plateau of ties, an all-negative window, N > 1."""
    N = 3
    x = _lp_rand((N, H, W, C), dt, 5)
    x[0, :min(H, 6), :min(W, 6), :8] = 0.0                     # plateau: the first maximum takes the gradient
    x[1, :3, :3, :] = -x[1, :3, :3, :].abs() - 0.5           # all-negative first window (ordinary negatives: above -3.0e38)
    _maxpool_case(lib, dt, N, H, W, C, c0, ld_x, ld_y, x)


def test_maxpool_second_grid_trip(lib):
    """N = 8, 73 x 73, C = 1024: 1.33 M forward and 5.5 M backward work items against the 1 048 576 threads of the capped grid."""
    N, H, W, C = 8, 73, 73, 1024
    assert N * 36 * 36 * C // 8 > GRID_CAP and N * H * W * C // 8 > GRID_CAP
    x = _lp_rand((N, H, W, C), BF, 5)
    OH = OW = 36
    xd = x.cuda()
    yd = torch.zeros(N, OH, OW, C, dtype=torch.bfloat16, device="cuda")
    amax = torch.full((N, OH, OW, C), 255, dtype=torch.uint8, device="cuda")
    _lib.check(lib.fn_maxpool3x3s2_fwd(ptr(xd), C, ptr(yd), C, N, H, W, C, ptr(amax), BF, stream()))
    dy = _lp_rand((N, OH, OW, C), BF, 6)
    dyd = dy.cuda()
    dx = [bitpattern((N, H, W, C), BF), bitpattern((N, H, W, C), BF)]
    _lib.check(lib.fn_maxpool3x3s2_bwd(ptr(xd), C, ptr(dyd), C, ptr(dx[0]), C, N, H, W, C, None, 0, BF, stream()))
    _lib.check(lib.fn_maxpool3x3s2_bwd(None, C, ptr(dyd), C, ptr(dx[1]), C, N, H, W, C, ptr(amax), 0, BF, stream()))
    torch.cuda.synchronize()
    assert torch.equal(dx[0], dx[1])
    y_c, am_c, dx_c = yd.cpu(), amax.cpu(), dx[0].cpu()
    for n in range(N):                                        # image by image: the window stack of the whole tensor is 3 GB
        want_y, want_am = eo.maxpool_ref(x[n:n + 1])
        assert same_bits(y_c[n:n + 1], want_y) and torch.equal(am_c[n:n + 1], want_am), n
        ref, absref = eo.maxpool_bwd_ref(dy[n:n + 1], want_am, H, W)
        assert_elementwise(dx_c[n:n + 1], ref, absref, 4, BF, f"maxpool dx image {n}")


# ---- global average pool ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("N", [1, 90])
@pytest.mark.parametrize("C", [8, 1536, 1792])
@pytest.mark.parametrize("HW", [1, 9, 64])                  # 64 = the 8 x 8 map of Inception-ResNet-v2
def test_avgpool_edges(lib, HW, C, N, dt):
    x = _lp_rand((N, HW, C), dt, 7, 1.0, 0.25)
    xd = x.cuda()
    y = bitpattern((N, C), dt)
    _lib.check(lib.fn_avgpool_fwd(ptr(xd), ptr(y), N, HW, C, dt, stream()))
    # HW adds from 0 (the first is exact), fl(1 / HW), the product: k = HW + 1
    assert_elementwise(y, x.double().mean(1), x.double().abs().mean(1), HW + 1, dt, "avgpool fwd")
    dy = _lp_rand((N, C), dt, 8)
    dyd = dy.cuda()
    dx = bitpattern((N, HW, C), dt)
    _lib.check(lib.fn_avgpool_bwd(ptr(dyd), ptr(dx), N, HW, C, dt, stream()))
    torch.cuda.synchronize()
    ref = (dy.double() / HW).view(N, 1, C).expand(N, HW, C)
    assert_elementwise(dx, ref, ref.abs(), 2, dt, "avgpool bwd")            # fl(1 / HW), the product
    assert same_bits(dx, dx[:, :1].expand(N, HW, C))         # every pixel receives the same bits


def test_avgpool3x3s1_second_grid_trip(lib):
    """N = 8, 35 x 35, C = 896: 1.10 M work items in forward and backward."""
    N, H, W, C, dt = 8, 35, 35, 896, BF
    assert N * H * W * C // 8 > GRID_CAP
    x = _lp_rand((N, H, W, C), dt, 21)
    xd = x.cuda()
    y = bitpattern((N, H, W, C), dt)
    _lib.check(lib.fn_avgpool3x3s1_fwd(ptr(xd), C, ptr(y), C, N, H, W, C, dt, stream()))
    ref, absref = eo.avgpool3s1_ref(x)
    assert_elementwise(y, ref, absref, 11, dt, "avgpool3x3s1 fwd")
    # backward: dx(i) = sum over the <= 9 outputs o covering i of dy(o) / taps(o): the gather form of the same stencil
    dy = _lp_rand((N, H, W, C), dt, 22)
    dyd = dy.cuda()
    dx = bitpattern((N, H, W, C), dt)
    _lib.check(lib.fn_avgpool3x3s1_bwd(ptr(dyd), C, ptr(dx), C, N, H, W, C, 0, dt, stream()))
    torch.cuda.synchronize()
    ty = torch.tensor([(i > 0) + 1 + (i + 1 < H) for i in range(H)], dtype=torch.float64).view(1, H, 1, 1)
    tx = torch.tensor([(i > 0) + 1 + (i + 1 < W) for i in range(W)], dtype=torch.float64).view(1, 1, W, 1)
    taps = ty * tx
    r, a = eo.avgpool3s1_ref((dy.double() / taps))            # the stencil sum, then undo the helper's own division
    assert_elementwise(dx, r * taps, a * taps, 11, dt, "avgpool3x3s1 bwd")    # per tap fl(1 / taps) and the product, then <= 9 adds


def test_dropout_second_grid_trip(lib):
    """N = 4200, C = 2048: 1.075 M work items; mask, scale and the zeroes bit for bit (one product, one rounding)."""
    N, C, keep, dt = 4200, 2048, 0.8, BF
    assert N * C // 8 > GRID_CAP
    x = _lp_rand((N, C), dt, 23)
    xd = x.cuda()
    step = torch.tensor([5], dtype=torch.int32, device="cuda")
    for fn in (lib.fn_dropout_fwd, lib.fn_dropout_bwd):
        y = bitpattern((N, C), dt)
        _lib.check(fn(ptr(xd), ptr(y), N, C, keep, 7, 1, ptr(step), dt, stream()))
        torch.cuda.synchronize()
        mask = torch.from_numpy(ro.dropout_mask(7, 1, 5, N, C, keep))
        inv = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(keep, dtype=torch.float32)
        want = torch.where(mask, x.float() * inv, torch.zeros(())).to(lp_dtype(dt))
        assert same_bits(y, want)


# ---- embedding head -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,E", [(9, 128), (90, 512), (5, 72), (2, 8)])       # E = 72, 8: idle tail lanes of the 64-wide workgroup / wave
def test_head_bn_edges(lib, N, E):
    g = torch.Generator().manual_seed(E)
    y = torch.randn(N, E, generator=g) * 3.0 + 1.5
    beta = torch.randn(E, generator=g) * 0.2
    mm0, mv0 = torch.randn(E, generator=g) * 0.1, torch.rand(E, generator=g) + 0.5
    yd, beta_d = y.cuda(), beta.cuda()
    for training in (1, 0):
        mm, mv = mm0.cuda(), mv0.cuda()
        out = torch.full((N, E), 7.0, device="cuda")
        sm, sr = torch.zeros(E, device="cuda"), torch.zeros(E, device="cuda")
        _lib.check(lib.fn_head_bn_fwd(ptr(yd), ptr(out), N, E, ptr(beta_d), ptr(mm), ptr(mv), ptr(sm), ptr(sr), training, 0.99, 1e-3, stream()))
        torch.cuda.synchronize()
        ref = eo.head_bn_ref(y, beta, mm0, mv0, training, 0.99, 1e-3)
        eo.check_bound(out, ref["out"], ref["e_out"], f"head_bn out training={training}")
        eo.check_bound(sm, ref["mean"], ref["e_mean"], "save_mean")
        eo.check_bound(sr, ref["rstd"], ref["e_rstd"], "save_rstd")
        if training:
            want, bound = eo.bn_moving_ref(mm0, ref["mean"], ref["e_mean"], 0.99)
            eo.check_bound(mm, want, bound, "head moving_mean")
            want, bound = eo.bn_moving_ref(mv0, ref["var"], ref["e_var"], 0.99)
            eo.check_bound(mv, want, bound, "head moving_var")
        else:
            assert torch.equal(mm.cpu(), mm0) and torch.equal(mv.cpu(), mv0)
    # backward from the saved statistics of the training pass, into both storage types
    mm, mv = mm0.cuda(), mv0.cuda()
    _lib.check(lib.fn_head_bn_fwd(ptr(yd), ptr(out), N, E, ptr(beta_d), ptr(mm), ptr(mv), ptr(sm), ptr(sr), 1, 0.99, 1e-3, stream()))
    dout = torch.randn(N, E, generator=g)
    dd = dout.cuda()
    for dt in DTS:
        dbeta0 = torch.linspace(-1, 1, E)
        dbeta = dbeta0.cuda()
        dy = bitpattern((N, E), dt)
        _lib.check(lib.fn_head_bn_bwd(ptr(dd), ptr(yd), ptr(sm), ptr(sr), ptr(dbeta), ptr(dy), N, E, dt, stream()))
        torch.cuda.synchronize()
        r, a, k, db, dba = eo.head_bn_bwd_ref(dout, y, sm.cpu(), sr.cpu(), N)
        assert_elementwise(dy, r, a, k, dt, "head_bn dy")
        assert_elementwise(dbeta, dbeta0.double() + db, dbeta0.double().abs() + dba, N + 1, dt, "head_bn dbeta", out_f32=True)


@pytest.mark.parametrize("N,E", [(9, 128), (90, 512), (5, 72), (2, 8)])
def test_l2norm_edges(lib, N, E):
    """Both sides of the clamp in one batch (N >= 4): an all-zero row, sum x^2 = eps / 100, sum x^2 = 100 eps."""
    x, dout = eo.l2norm_inputs(N, E, seed=E)
    xd, dd = x.cuda(), dout.cuda()
    out = torch.full((N, E), 7.0, device="cuda")
    _lib.check(lib.fn_l2norm_fwd(ptr(xd), ptr(out), N, E, 1e-10, stream()))
    ref, bound, s, e_s = eo.l2norm_ref(x, 1e-10)
    eo.check_bound(out, ref, bound, "l2norm fwd")
    dx = torch.full((N, E), 7.0, device="cuda")
    _lib.check(lib.fn_l2norm_bwd(ptr(xd), ptr(dd), ptr(dx), N, E, 1e-10, stream()))
    torch.cuda.synchronize()
    r, b, margin_ok = eo.l2norm_bwd_ref(x, dout, 1e-10)
    assert margin_ok, "a row whose clamp decision is ambiguous in fp32"
    eo.check_bound(dx, r, b, "l2norm bwd")
    if N >= 4:
        assert float(out[0].abs().max()) == 0 and bool((s[:2] < 1e-10).all()) and bool((s[2:] > 1e-10).all())


# ---- data movement ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
def test_cast_f32_to_lp_edges(lib, dt):
    """Ties, f16 subnormals, the largest finite value and the first that rounds to infinity, +-0, +-Inf, NaN; n = 1, 257 and a
    second grid trip."""
    lp = lp_dtype(dt)
    fin = torch.finfo(lp)
    ulp1 = 2.0 ** -7 if dt == BF else 2.0 ** -10
    special = [0.0, -0.0, float("inf"), float("-inf"), float("nan"), 1.0 + ulp1 / 2, 1.0 + 3 * ulp1 / 2, -(1.0 + ulp1 / 2), 1.0 + ulp1 / 2 + 2.0 ** -23,
               fin.max, fin.max * (1 + ulp1 / 4), fin.max * (1 + ulp1 / 2), -fin.max * (1 + ulp1 / 2), 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25, 2.0 ** -25 * (1 + 2.0 ** -20),
               6.0e-8, 5.9e-6, 2.0 ** -14, 2.0 ** -14 * (1 - 2.0 ** -12), 2.0 ** -126]
    # bf16: the midpoint between the largest finite value and 2^128 (rounds to infinity) and the fp32 value just below it; f16: 65520
    # and the value just below it
    special += torch.tensor([0x7F7F8000, 0x7F7F7FFF, 0x477FF000, 0x477FEFFF], dtype=torch.int32).view(torch.float32).tolist()
    for n in (1, 257, GRID_CAP + 300):
        g = torch.Generator().manual_seed(n)
        x = torch.randn(n, generator=g) * 100
        m = min(n, len(special))
        x[n - m:] = torch.tensor(special[:m])                # the specials sit in the tail: the second trip for the largest n
        xd = x.cuda()
        y = bitpattern((n + 8,), dt)
        before = y.clone()
        _lib.check(lib.fn_cast_f32_to_lp(ptr(xd), ptr(y), n, dt, stream()))
        torch.cuda.synchronize()
        want = x.to(lp)
        got = y[:n].cpu()
        nan = torch.isnan(want)
        assert torch.equal(torch.isnan(got), nan)            # NaN stays NaN (payloads may differ)
        assert same_bits(got[~nan], want[~nan])
        assert same_bits(y[n:], before[n:])


@pytest.mark.parametrize("bits", [20, 40])
def test_acc_to_float_edges(lib, bits):
    for n in (1, 257, GRID_CAP + 300):
        g = torch.Generator().manual_seed(n)
        src = torch.randint(-(1 << 50), 1 << 50, (n,), generator=g, dtype=torch.int64)
        special = torch.tensor([1 << 62, -(1 << 62), (1 << 62) + 12345, -1, 0, 1, (1 << 53) + 1, -(1 << 53) - 1], dtype=torch.int64)
        m = min(n, len(special))
        src[n - m:] = special[:m]
        sd = src.cuda()
        dst = torch.full((n + 4,), 7.0, device="cuda")
        _lib.check(lib.fn_acc_to_float(ptr(sd), ptr(dst), n, bits, stream()))
        torch.cuda.synchronize()
        want = (src.numpy().astype(np.float64) * 2.0 ** -bits).astype(np.float32)
        assert np.array_equal(dst[:n].cpu().numpy(), want)
        assert float(dst[n:].min()) == 7.0 and float(dst[n:].max()) == 7.0


@pytest.mark.parametrize("nbytes", [16, 76800])
def test_gather_images_edges(lib, nbytes):
    """Repeated and out-of-order indices, bit for bit; the pool and the bytes after the output stay as they were."""
    rng = np.random.default_rng(nbytes)
    pool = torch.from_numpy(rng.integers(0, 256, (7, nbytes), dtype=np.uint8))
    idx = torch.tensor([6, 0, 3, 3, 1, 6, 5, 0, 2], dtype=torch.int32)
    pd, idd = pool.cuda(), idx.cuda()
    out = torch.full((len(idx) + 1, nbytes), 0xA5, dtype=torch.uint8, device="cuda")
    _lib.check(lib.fn_gather_images(ptr(pd), ptr(idd), ptr(out), len(idx), nbytes, stream()))
    torch.cuda.synchronize()
    assert torch.equal(out[:len(idx)].cpu(), pool[idx.long()])
    assert bool((out[len(idx)] == 0xA5).all()) and torch.equal(pd.cpu(), pool)


def test_gather_images_rejects_a_size_that_is_not_whole_vectors(lib):
    """299 x 299 x 3 = 268 203 bytes: refused on the host, with the cause in the message; the miner refuses it when it is built."""
    from facenet_amd.train import check_gather_bytes
    t = torch.zeros(64, dtype=torch.uint8, device="cuda")
    i = torch.zeros(1, dtype=torch.int32, device="cuda")
    for nbytes in (299 * 299 * 3, 8, 17):
        with pytest.raises(ValueError, match="not a multiple of 16"):
            _lib.check(lib.fn_gather_images(ptr(t), ptr(i), ptr(t), 1, nbytes, stream()))
        with pytest.raises(ValueError, match="not a multiple of 16"):
            check_gather_bytes(nbytes)
    assert check_gather_bytes(160 * 160 * 3) == 76800


# ---- image ops ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src_f32", [0, 1])
@pytest.mark.parametrize("H,W", [(160, 160), (182, 150), (64, 96), (299, 299)])
def test_image_resize_bilinear_edges(lib, H, W, src_f32):
    """u8 and fp32 sources; the identity bit for bit; down- and up-scaling against the fp64 half-pixel rule with the position error
    in the bound (64 x 96 has source positions that are exactly integral)."""
    N, OH, OW = 3, 160, 160
    rng = np.random.default_rng(H * 1000 + W)
    if src_f32:
        img = torch.from_numpy((rng.normal(size=(N, H, W, 3)) * 60 + 100).astype(np.float32))
    else:
        img = torch.from_numpy(rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8))
    d = img.cuda()
    out = torch.full((N * OH * OW * 3 + 4,), 7.0, device="cuda")
    _lib.check(lib.fn_image_resize_bilinear(ptr(d), src_f32, ptr(out), N, H, W, OH, OW, stream()))
    torch.cuda.synchronize()
    got = out[:-4].view(N, OH, OW, 3).cpu()
    assert float(out[-4:].min()) == 7.0 and float(out[-4:].max()) == 7.0
    if (H, W) == (OH, OW):
        assert torch.equal(got, img.float())
    ref, bound = eo.resize_ref(img, OH, OW)
    eo.check_bound(got, ref, bound, f"resize {H}x{W}")


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("HW", [100, 160 * 160])           # 100: 300 values, not a multiple of 256 nor of the 16-byte vector
def test_image_normalize_edges(lib, HW, mode, dt):
    """u8 and fp32 (negative, non-integer) input, both modes and storage types, a constant image (exactly 0 in both modes: the sums of
    a constant u8 image are exact, mode 1 divides by the 1/sqrt(numel) clamp), channels 3..7 exactly zero."""
    N = 3
    rng = np.random.default_rng(HW + mode)
    u8 = rng.integers(0, 256, (N, HW, 3), dtype=np.uint8)
    u8[1] = 77
    f32 = (rng.normal(size=(N, HW, 3)) * 40 - 7.3).astype(np.float32)
    work = torch.zeros(8 * N, dtype=torch.float32, device="cuda")
    for src, fn in ((torch.from_numpy(u8), lib.fn_image_normalize), (torch.from_numpy(f32), lib.fn_image_normalize_f32)):
        d = src.cuda()
        out = bitpattern((N, HW, 8), dt)
        _lib.check(fn(ptr(d), ptr(out), ptr(work), N, HW, mode, dt, stream()))
        torch.cuda.synchronize()
        ref, bound = eo.normalize_ref(src[[0, 2]], mode)
        got = out.cpu()
        eo.check_bound(got[[0, 2], :, :3], ref, bound + eo.U_LP[dt] * (ref.abs() + bound) + eo.ETA_LP[dt], f"normalize mode {mode}")
        assert float(got[..., 3:].float().abs().max()) == 0
        if src.dtype == torch.uint8:
            assert float(got[1].float().abs().max()) == 0, "constant image"
        else:
            ref1, bound1 = eo.normalize_ref(src[1:2], mode)
            eo.check_bound(got[1:2, :, :3], ref1, bound1 + eo.U_LP[dt] * (ref1.abs() + bound1) + eo.ETA_LP[dt], f"normalize mode {mode}")
