"""The references and bounds of tests/elementwise_oracle.py checked against each other, without a GPU: on the inputs of the GPU
edge cases an fp32 restatement of every formula (correctly rounded 1/sqrt, exp, log) must stay inside the bound the GPU test
applies, and a deliberately wrong restatement -- one element of a tail stripe zeroed, one row of a second loop trip skipped, one
replica dropped, one column of a second softmax trip left out -- must fall outside it.  The same module records the error of the
restatement's 1/sqrt, exp and log in fp32 ulps, from which the ulp slack of the device functions is fixed (4 x, at least 4)."""
import numpy as np
import pytest
import torch

from tests import elementwise_oracle as eo
from tests.util import assert_acc_sums, assert_elementwise

BF, HF = eo.BF, eo.HF
BN_CASES = [c for c in eo.bn_cases()]
SOFTMAX_CASES = [(6, 37, 40, 40), (90, 1000, 1000, 1008), (7, 8631, 8640, 8632)]
HEAD_CASES = [(9, 128), (90, 512), (5, 72), (2, 8)]
TRIPLET_CASES = [(1, 128), (7, 128), (30, 512), (5, 8)]


def _bn_seed(name):
    return sum(name.encode()) % 1000


def test_ulp_slack_constants_come_from_the_restatement_error():
    """c = max(4, 4 x the largest fp32-restatement error in ulps) for rsqrtf, __expf, logf on the GPU cases' inputs."""
    worst = {"rsqrt": 0.0, "exp": 0.0, "log": 0.0}
    for name, M, C, c0, ld_y, ld_z, reps, relu, moving, reduced, far in BN_CASES:
        for dt in (BF, HF):
            y, dz, beta, S1, S2 = eo.bn_inputs(dt, M, C, _bn_seed(name), far)
            t32 = eo.bn_affine_f32(S1, S2, M, 1e-3, beta)[4]
            worst["rsqrt"] = max(worst["rsqrt"], float(eo.ulps(eo._rsqrt32(t32), t32.astype(np.float64) ** -0.5).max()))
    for N, C, ld, ld_d in SOFTMAX_CASES:
        x, labels = eo.softmax_inputs(N, C, ld, seed=N)
        _, _, _, aux = eo.softmax_f32(x, labels, C, 1.0 / N, BF)
        a64 = aux["a"].astype(np.float64)
        # the exp of the fp32 argument a: the argument's own rounding is accounted separately in softmax_ref
        worst["exp"] = max(worst["exp"], float(eo.ulps(aux["e"], np.exp(a64)).max()))
        worst["log"] = max(worst["log"], float(eo.ulps(aux["lse"], np.log(aux["s"].astype(np.float64))).max()))
    for N, E in HEAD_CASES:
        x, _ = eo.l2norm_inputs(N, E, seed=E)
        _, s = eo.l2norm_f32(x, 1e-10)
        t = np.maximum(s, np.float32(1e-10))
        worst["rsqrt"] = max(worst["rsqrt"], float(eo.ulps(eo._rsqrt32(t), t.astype(np.float64) ** -0.5).max()))
    print("fp32 restatement error in ulps:", worst)
    assert 0 < worst["rsqrt"] <= 0.5001 and 0 < worst["exp"] <= 0.5001 and 0 < worst["log"] <= 0.5001, worst
    assert eo.C_RSQRT == max(4, int(np.ceil(4 * worst["rsqrt"])))
    assert eo.C_EXP == max(4, int(np.ceil(4 * worst["exp"])))
    assert eo.C_LOG == max(4, int(np.ceil(4 * worst["log"])))


@pytest.mark.parametrize("dt", [BF, HF])
@pytest.mark.parametrize("case", BN_CASES, ids=[c[0] for c in BN_CASES])
def test_bn_restatement_inside_bounds_and_planted_errors_outside(case, dt):
    name, M, C, c0, ld_y, ld_z, reps, relu, moving, reduced, far = case
    y, dz, beta, S1, S2 = eo.bn_inputs(dt, M, C, _bn_seed(name), far)
    # stage 1: scale, shift, moving statistics from the exact sums
    ref = eo.bn_affine_ref(S1, S2, M, 1e-3, beta)
    sc, sh, mean, var, _ = eo.bn_affine_f32(S1, S2, M, 1e-3, beta)
    for key, got in (("scale", sc), ("shift", sh), ("mean", mean), ("var", var)):
        eo.check_bound(torch.from_numpy(got), ref[key], ref["e_" + key], f"{name} {key}")
    mm0, mv0 = torch.linspace(-1, 1, C), torch.linspace(0.5, 2, C)
    for batch, e_batch, old, got_b in ((ref["mean"], ref["e_mean"], mm0, mean), (ref["var"], ref["e_var"], mv0, var)):
        want, bound = eo.bn_moving_ref(old, batch, e_batch, 0.99)
        eo.check_bound(torch.from_numpy(eo.bn_moving_f32(old.numpy(), got_b, 0.99)), want, bound, f"{name} moving")
    # one replica dropped: far outside the bound of the scale or the shift
    if reps > 1:
        p1, p2 = eo.split_replicas(S1, reps, 1), eo.split_replicas(S2, reps, 2)
        sc_bad, sh_bad = eo.bn_affine_f32(p1[:-1].sum(0), p2[:-1].sum(0).abs(), M, 1e-3, beta)[:2]
        assert not eo.inside(torch.from_numpy(sc_bad), ref["scale"], ref["e_scale"]) or not eo.inside(torch.from_numpy(sh_bad), ref["shift"], ref["e_shift"])
    # stage 2 from the fp32 scale / shift (the inputs of these formulas)
    sc32, sh32 = torch.from_numpy(sc), torch.from_numpy(sh)
    assert eo.bn_zero_margin(y, sc32, sh32) == 0            # no ambiguous ReLU decision
    z = eo.bn_fwd_f32(y, sc32, sh32, relu, dt)
    zr, za, k = eo.bn_fwd_ref(y, sc32, sh32, relu)
    assert_elementwise(z, zr, za, k, dt, f"{name} z")
    # one element of the tail stripe zeroed
    tail = 64 * ((C - 1) // 64)
    col = tail + int(zr[:, tail:].abs().amax(0).argmax())
    row = int(zr[:, col].abs().argmax())
    assert float(zr[row, col].abs()) > 1e-2
    z_bad = z.clone()
    z_bad[row, col] = 0
    with pytest.raises(AssertionError):
        assert_elementwise(z_bad, zr, za, k, dt, "planted")
    # backward sums in the reduce kernel's chunking
    A1, A2 = eo.bn_sums_f32(dz, y, sc32, sh32, beta, relu, M, C)
    r1, a1, r2, a2, te2 = eo.bn_sums_ref(dz, y, sc32, sh32, beta, relu)
    rows, tiles = eo.reduce_chain(M, C)
    assert_acc_sums(A1, r1, a1, eo.ACC_GRAD_BITS, tiles, f"{name} sum dyh", rows=rows)
    assert_acc_sums(A2, r2, a2, eo.ACC_GRAD_BITS, tiles, f"{name} sum dyh xhat", term_err=te2, rows=rows)
    # one row skipped: a row of the second four-row trip where there is one, otherwise the last row
    rpb = eo.reduce_rows_per_block(M, C)
    skip = min(M - 1, 4 * 32 + 3) if rpb > 128 else M - 1
    B1, B2 = eo.bn_sums_f32(dz, y, sc32, sh32, beta, relu, M, C, skip_row=skip)
    with pytest.raises(AssertionError):
        assert_acc_sums(B1, r1, a1, eo.ACC_GRAD_BITS, tiles, "planted", rows=rows)
    # dz from the exact integer sums
    dy = eo.bn_bwd_f32(dz, y, sc32, sh32, beta, A1, A2, M, relu, dt)
    dr, da, kb = eo.bn_bwd_ref(dz, y, sc32, sh32, beta, A1, A2, M, relu)
    assert_elementwise(dy, dr, da, kb, dt, f"{name} dz")
    dy_bad = dy.clone()
    row = int(dr[:, col].abs().argmax())
    dy_bad[row, col] = 0
    with pytest.raises(AssertionError):
        assert_elementwise(dy_bad, dr, da, kb, dt, "planted")


@pytest.mark.parametrize("N,C,ld,ld_d", SOFTMAX_CASES)
def test_softmax_restatement_inside_bounds_and_planted_error_outside(N, C, ld, ld_d):
    x, labels = eo.softmax_inputs(N, C, ld, seed=N)
    ref = eo.softmax_ref(x, labels, C, 1.0 / N)
    for dt in (BF, HF):
        loss, g, dbias, _ = eo.softmax_f32(x, labels, C, 1.0 / N, dt)
        eo.check_bound(torch.tensor(float(loss)), ref["loss"], ref["e_loss"], "loss")
        eo.check_bound(g, ref["g"], ref["e_g"] + eo.U_LP[dt] * (ref["g"].abs() + ref["e_g"]) + eo.ETA_LP[dt], "dlogits")
        eo.check_bound(dbias.double() * 2.0 ** -eo.ACC_GRAD_BITS, ref["dbias"], ref["e_dbias"], "dbias")
    # the column holding a row's largest logit left out of the sum (for C > 256 a column of the second trip exists; the largest one
    # is used because a small one vanishes in the storage rounding, as it would on the device)
    col = int(x[0, :C].argmax())
    loss_bad = eo.softmax_f32(x, labels, C, 1.0 / N, BF, skip_col=col)[0]
    assert not eo.inside(torch.tensor(float(loss_bad)), ref["loss"], ref["e_loss"])
    # the loss bound is tight enough to see one fp32-visible error: a relative change of 1e-5 of one row's term
    assert float(ref["e_loss"]) < 1e-5 * float(ref["loss"].abs()) + 1e-6


@pytest.mark.parametrize("N,E", HEAD_CASES)
def test_head_restatements_inside_bounds(N, E):
    g = torch.Generator().manual_seed(E)
    y = torch.randn(N, E, generator=g) * 3.0 + 1.5
    beta = torch.randn(E, generator=g) * 0.2
    mm, mv = torch.randn(E, generator=g) * 0.1, torch.rand(E, generator=g) + 0.5
    for training in (1, 0):
        ref = eo.head_bn_ref(y, beta, mm, mv, training, 0.99, 1e-3)
        out, mean, var, rstd = eo.head_bn_f32(y, beta, mm, mv, training, 1e-3)
        eo.check_bound(torch.from_numpy(out), ref["out"], ref["e_out"], "head out")
        eo.check_bound(torch.from_numpy(rstd), ref["rstd"], ref["e_rstd"], "head rstd")
        eo.check_bound(torch.from_numpy(mean), ref["mean"], ref["e_mean"], "head mean")
        eo.check_bound(torch.from_numpy(var), ref["var"], ref["e_var"], "head var")
        bad = out.copy()
        bad[N - 1, E - 1] = 0                               # the last lane of the tail workgroup
        assert not eo.inside(torch.from_numpy(bad), ref["out"], ref["e_out"])
    x, dout = eo.l2norm_inputs(N, E, seed=E)
    outr, bound, s, e_s = eo.l2norm_ref(x, 1e-10)
    out32, s32 = eo.l2norm_f32(x, 1e-10)
    eo.check_bound(torch.from_numpy(out32), outr, bound, "l2norm")
    eo.check_bound(torch.from_numpy(s32).view(-1, 1), s, e_s, "sum x^2")
    _, _, margin_ok = eo.l2norm_bwd_ref(x, dout, 1e-10)
    assert margin_ok
    bad = out32.copy()
    bad[N - 1, E - 1] *= 1 + 2e-5
    assert not eo.inside(torch.from_numpy(bad), outr, bound)


@pytest.mark.parametrize("T,E", TRIPLET_CASES)
def test_triplet_restatement_inside_bounds_and_hinges_unambiguous(T, E):
    for alpha in (0.2, 0.0):
        emb = eo.triplet_inputs(T, E, alpha, seed=T)
        ref = eo.triplet_ref(emb, T, E, alpha)
        # no ambiguous hinge: |l| above its fp32 error, or p == n bit for bit (pos and neg are then the same fp32 number)
        clear = (ref["l"].abs() > ref["e_l"]) | (ref["same"] & (alpha == 0.0))
        assert bool(clear.all()), (ref["l"], ref["e_l"])
        loss, grad, l32 = eo.triplet_f32(emb, T, E, alpha)
        eo.check_bound(torch.tensor(float(loss)), ref["loss"], ref["e_loss"], "triplet loss")
        eo.check_bound(torch.from_numpy(grad), ref["grad"], ref["e_grad"], "triplet grad")
        if alpha == 0.0:
            assert l32[T - 1] == 0 and not grad[3 * (T - 1):].any()
        if T > 1:       # one active triplet dropped from the loss
            assert not eo.inside(torch.tensor(float(loss) - float(ref["l"][0].clamp(min=0)) / T), ref["loss"], ref["e_loss"])


def test_resize_and_normalize_bounds_hold_for_an_fp32_restatement():
    f = np.float32
    rng = np.random.default_rng(0)
    for (H, W) in ((160, 160), (182, 150), (64, 96), (299, 299)):
        img = torch.from_numpy(rng.integers(0, 256, (2, H, W, 3)).astype(np.float32))
        ref, bound = eo.resize_ref(img, 160, 160)
        x = img.numpy()
        sy, sx = f(H) / f(160), f(W) / f(160)
        fy = (np.arange(160, dtype=f) + f(0.5)) * sy - f(0.5)
        fx = (np.arange(160, dtype=f) + f(0.5)) * sx - f(0.5)
        y0, y1 = np.maximum(np.floor(fy).astype(int), 0), np.minimum(np.ceil(fy).astype(int), H - 1)
        x0, x1 = np.maximum(np.floor(fx).astype(int), 0), np.minimum(np.ceil(fx).astype(int), W - 1)
        ly, lx = (fy - np.floor(fy)).reshape(1, 160, 1, 1), (fx - np.floor(fx)).reshape(1, 1, 160, 1)
        top = x[:, y0][:, :, x0] + (x[:, y0][:, :, x1] - x[:, y0][:, :, x0]) * lx
        bot = x[:, y1][:, :, x0] + (x[:, y1][:, :, x1] - x[:, y1][:, :, x0]) * lx
        out = top + (bot - top) * ly
        eo.check_bound(torch.from_numpy(out), ref, bound, f"resize {H}x{W}")
        if (H, W) == (160, 160):
            assert np.array_equal(out, x)
        bad = out.copy()
        bad[1, 159, 159, 2] += 0.01 * (1 + abs(bad[1, 159, 159, 2]))
        assert not eo.inside(torch.from_numpy(bad), ref, bound)
    for mode in (0, 1):
        img = torch.from_numpy(rng.normal(size=(2, 100, 3)).astype(f) * 40 - 7.3)
        ref, bound = eo.normalize_ref(img, mode)
        x = img.numpy()
        if mode == 0:
            mx, mn = x.max((1, 2), keepdims=True), x.min((1, 2), keepdims=True)
            out = (f(2) * x - (mn + mx)) / np.maximum(mx - mn, f(1e-3))
        else:
            cnt = f(300)
            mean = x.sum((1, 2), keepdims=True, dtype=f) / cnt
            var = np.maximum((x * x).sum((1, 2), keepdims=True, dtype=f) / cnt - mean * mean, f(0))
            out = (x - mean) / np.maximum(np.sqrt(var), eo._rsqrt32(np.array(cnt)))
        eo.check_bound(torch.from_numpy(out), ref, bound, f"normalize mode {mode}")
        assert float(bound.max()) < 1e-4                   # far below the storage rounding: the per-element check decides


def test_host_side_rejections_need_no_gpu():
    """A pool of one identity and an image size that is not whole 16-byte vectors are refused before anything is launched."""
    from facenet_amd.train import check_gather_bytes
    from facenet_amd.triplet import select_triplets
    with pytest.raises(ValueError, match="at least two identities"):
        select_triplets(torch.zeros(6, 6), np.full(6, 3), 0.2, 2)
    with pytest.raises(ValueError, match="not a multiple of 16"):
        check_gather_bytes(299 * 299 * 3)
    assert check_gather_bytes(160 * 160 * 3) == 76800


@pytest.mark.parametrize("N,E", HEAD_CASES)
def test_head_backward_restatements_inside_bounds(N, E):
    f = np.float32
    g = torch.Generator().manual_seed(E)
    y = torch.randn(N, E, generator=g) * 3.0 + 1.5
    beta = torch.zeros(E)
    _, mean, _, rstd = eo.head_bn_f32(y, beta, None, None, 1, 1e-3)
    dout = torch.randn(N, E, generator=g)
    yn, gn = y.numpy().astype(f), dout.numpy().astype(f)
    s1, s2 = np.zeros(E, f), np.zeros(E, f)
    for n in range(N):
        s1 = s1 + gn[n]
        s2 = s2 + gn[n] * (yn[n] - mean) * rstd
    k1, k2 = s1 / f(N), s2 / f(N)
    dy = rstd * (gn - k1 - (yn - mean) * rstd * k2)
    for dt in (BF, HF):
        r, a, k, db, dba = eo.head_bn_bwd_ref(dout, y, torch.from_numpy(mean), torch.from_numpy(rstd), N)
        assert_elementwise(torch.from_numpy(dy).to(eo.lp_torch(dt)), r, a, k, dt, "head_bn dy")
        assert_elementwise(torch.from_numpy(s1), db, dba, N + 1, dt, "head_bn dbeta", out_f32=True)
        bad = torch.from_numpy(dy).to(eo.lp_torch(dt)).clone()
        i = int(r[:, E - 1].abs().argmax())
        bad[i, E - 1] = 0
        with pytest.raises(AssertionError):
            assert_elementwise(bad, r, a, k, dt, "planted")
    # l2norm backward in the kernel's order
    x, dout = eo.l2norm_inputs(N, E, seed=E)
    xn, gn = x.numpy().astype(f), dout.numpy().astype(f)
    pad = lambda v: np.pad(v, ((0, 0), (0, eo.cdiv(E, 64) * 64 - E))).reshape(N, -1, 64)
    s, d = np.zeros((N, 64), f), np.zeros((N, 64), f)
    for t in range(pad(xn).shape[1]):
        s = s + pad(xn)[:, t] * pad(xn)[:, t]
        d = d + pad(xn)[:, t] * pad(gn)[:, t]
    from oracle import facenet_oracle as fo
    s, d = fo._wave_sum32(s)[:, None], fo._wave_sum32(d)[:, None]
    rr = eo._rsqrt32(np.maximum(s, f(1e-10)))
    dx = np.where(s < f(1e-10), rr * gn, rr * (gn - xn * rr * rr * d))
    ref, bound, margin_ok = eo.l2norm_bwd_ref(x, dout, 1e-10)
    assert margin_ok
    eo.check_bound(torch.from_numpy(dx), ref, bound, "l2norm bwd")
    bad = dx.copy()
    bad[N - 1, E - 1] += 1e-4 * (1 + abs(bad[N - 1, E - 1]))
    assert not eo.inside(torch.from_numpy(bad), ref, bound)
