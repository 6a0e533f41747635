"""The kernels of csrc/optim.hip at their edges, through the C ABI, element by element against fp64 or bit for bit (references
and bounds: tests/optim_oracle.py; the bounds themselves are checked in tests/test_optim_refs_host.py).

  * fn_adam_keras / fn_adam_keras_ema: one step from a given fp32 state (re-uploaded before every step), m, v and w bounded at
    every element; the L2 boundary inside a float4; n_lp = 0 / partial / n; both dtypes; t up to where the beta powers are
    subnormal or zero; the pack bit-equal to round-to-nearest-even of the device's own w; all-zero segments stay bitwise +0;
    sentinels past n and n_lp survive; g is unchanged.
  * the second trip of the optimiser kernels' grid-stride loop (n > 4 * 4096 * 256), for Adam and for fn_opt_keras_ema.
  * fn_adam_tick against adam_beta_powers for t = 1 .. 2048, 10^4, 10^5, bit for bit.
  * fn_fold_bn on a synthetic table (offsets with gaps, bn = -1, fold_bias = -1, variances 0 .. 1e6, cancelling biases), with
    gx = 1 and past the grid cap; fn_pack_transpose bit for bit on a table that takes the 64 x 64 and the scalar path, with
    gx = 1 and at the grid cap.
  * rejected arguments return FN_EINVAL and write nothing."""
import numpy as np
import pytest
import torch

from facenet_amd import _lib
from facenet_amd.optimizers import OPTIMIZERS, adam_beta_powers
from tests import elementwise_oracle as eo
from tests import ema_oracle
from tests import optim_oracle as oo
from tests import optimizer_oracle
from tests.util import ptr, stream

pytestmark = pytest.mark.gpu
BF, HF = _lib.FN_BF16, _lib.FN_F16
DTS = [BF, HF]
F = np.float32
PAD, SENT = 8, np.float32(-1234.5)
FN_EINVAL = -1


def _dev(a):
    """n values followed by PAD sentinels: nothing may be written past n."""
    return torch.from_numpy(np.concatenate([np.asarray(a, dtype=F), np.full(PAD, SENT, F)])).cuda()


def _pattern(n, c=0x2B67):
    return torch.from_numpy((((np.arange(n, dtype=np.int64) * 25173 + c) & 0xFFFF).astype(np.uint16)).view(np.int16))


def _hyper(t, lr=oo.LR, gs=oo.GS):
    """hyper with word 4 = t - 1, ticked once on the device."""
    hyper = torch.tensor([lr, 1.0, 1.0, gs, 0.0, 0.0, 0.0, 0.0], device="cuda")
    hyper.view(torch.int32)[4:5].fill_(t - 1)
    _lib.check(_lib.load().fn_adam_tick(ptr(hyper), oo.BETA1, oo.BETA2, stream()), "adam_tick")
    return hyper


def _run_adam(lib, inp, n, n_decay, n_lp, t, dt, ema):
    """One step from the state `inp`, uploaded afresh.  Returns the read-back buffers (numpy, sentinels included)."""
    w, g, m, v, shadow = (_dev(inp[k]) for k in ("w", "g", "m", "v", "shadow"))
    wlp0 = _pattern(n + PAD)
    wlp = wlp0.cuda()
    hyper = _hyper(t)
    args = (ptr(w), ptr(g), ptr(m), ptr(v), None if n_lp is None else ptr(wlp), n_lp or 0, n, n_decay, ptr(hyper), oo.BETA1, oo.BETA2,
            oo.EPS, oo.L2, dt)
    if ema:
        _lib.check(lib.fn_adam_keras_ema(*args, ptr(shadow), oo.DECAY, stream()), "adam_keras_ema")
    else:
        _lib.check(lib.fn_adam_keras(*args, stream()), "adam_keras")
    torch.cuda.synchronize()
    out = {k: b.cpu().numpy() for k, b in (("w", w), ("g", g), ("m", m), ("v", v), ("shadow", shadow), ("wlp", wlp), ("hyper", hyper))}
    out["wlp0"] = wlp0.numpy()
    return out


def _check_adam(out, inp, n, n_decay, n_lp, t, dt, zero_segs, ties_at, what):
    hyper = out["hyper"]
    assert int(hyper.view(np.int32)[4]) == t
    want_b = np.array(adam_beta_powers(t, oo.BETA1, oo.BETA2), dtype=F)
    assert np.array_equal(hyper[1:3].view(np.uint32), want_b.view(np.uint32)), (what, hyper[1:3], want_b)
    assert hyper[0] == F(oo.LR) and hyper[3] == F(oo.GS) and not hyper[5:].any()
    # fp64 from the operands exactly as the kernel received them, the read-back hyper words among them
    ref = oo.adam_ref(inp["w"], inp["g"], inp["m"], inp["v"], hyper, n_decay)
    eo.check_bound(out["m"][:n], ref["m"], ref["e_m"], f"{what} m")
    eo.check_bound(out["v"][:n], ref["v"], ref["e_v"], f"{what} v")
    eo.check_bound(out["w"][:n], ref["w"], ref["e_w"], f"{what} w")
    assert np.array_equal(out["g"].view(np.int32)[:n], inp["g"].view(np.int32)), f"{what}: g changed"
    for k in ("w", "g", "m", "v"):
        assert np.all(out[k][n:] == SENT), f"{what}: {k} written past n"
    # the pack: round-to-nearest-even of the device's own w, bit for bit; nothing past n_lp
    n_pack = n_lp or 0
    assert np.array_equal(out["wlp"][:n_pack], oo.pack_rne(out["w"][:n_pack], dt)), f"{what}: pack"
    assert np.array_equal(out["wlp"][n_pack:], out["wlp0"][n_pack:]), f"{what}: pack written past n_lp"
    # all-zero segments stay bitwise +0 (what the padded classifier rows rely on)
    for lo, hi in zero_segs:
        for k in ("w", "m", "v"):
            assert not out[k][lo:hi].view(np.int32).any(), f"{what}: {k} of a zero segment"
        assert not out["wlp"][lo:min(hi, n_pack)].any(), f"{what}: pack of a zero segment"
    if n_decay <= ties_at:      # no gradient, no moment, no decay: the tie values reach the pack exactly as they were put in
        sl = slice(ties_at, ties_at + inp["n_ties"])
        assert np.array_equal(out["w"][sl].view(np.int32), inp["w"][sl].view(np.int32)), f"{what}: tie values moved"


def _check_ema(out, plain, inp, n, t, what):
    for k in ("w", "m", "v", "wlp", "g", "hyper"):
        a, b = out[k], plain[k]
        assert np.array_equal(a.view(np.int32) if a.dtype == F else a, b.view(np.int32) if b.dtype == F else b), f"{what}: {k} differs from plain Adam"
    want = ema_oracle.update(inp["shadow"], out["w"][:n], t, oo.DECAY)
    assert np.array_equal(out["shadow"][:n].view(np.int32), want.view(np.int32)), f"{what}: shadow"
    assert np.all(out["shadow"][n:] == SENT)
    assert np.all(plain["shadow"][:n] == inp["shadow"]), f"{what}: plain Adam touched the shadow"


# ---- 1. Adam, one step ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", oo.ADAM_TS)
@pytest.mark.parametrize("dt", DTS)
def test_adam_one_step_edges(lib, dt, t):
    """Every n_decay (0, n, 4j+1, 4j+2, 4j+3) with every n_lp (NULL, partial, n) at this dtype and step count, plain and fused
    with the moving average."""
    inp, n = oo.adam_inputs(), oo.ADAM_N
    for n_decay in oo.ADAM_N_DECAY:
        for n_lp in oo.ADAM_N_LP:
            what = f"dt {dt} t {t} n_decay {n_decay} n_lp {n_lp}"
            plain = _run_adam(lib, inp, n, n_decay, n_lp, t, dt, ema=False)
            _check_adam(plain, inp, n, n_decay, n_lp, t, dt, oo.ADAM_ZERO_SEGS, oo.ADAM_TIES, what)
            fused = _run_adam(lib, inp, n, n_decay, n_lp, t, dt, ema=True)
            _check_ema(fused, plain, inp, n, t, what)


# ---- 2. the second trip of the grid-stride loop ----------------------------------------------------------------------------------
@pytest.mark.parametrize("entry,dt", [("adam_keras", BF), ("adam_keras_ema", HF)])
def test_adam_second_trip_of_the_stride_loop(lib, entry, dt):
    """n = 4 (4096 * 256 + 257): the last 257 float4s are a second trip of the loop; the L2 boundary, the end of the pack, a
    zero segment and the tie values lie in it.  The same bounds over all elements."""
    inp, n, t = oo.stride_inputs(), oo.STRIDE_N, 3
    ema = entry == "adam_keras_ema"
    out = _run_adam(lib, inp, n, oo.STRIDE_N_DECAY, oo.STRIDE_N_LP, t, dt, ema)
    _check_adam(out, inp, n, oo.STRIDE_N_DECAY, oo.STRIDE_N_LP, t, dt, oo.STRIDE_ZERO_SEGS, oo.STRIDE_TIES, entry)
    if ema:
        want = ema_oracle.update(inp["shadow"], out["w"][:n], t, oo.DECAY)
        assert np.array_equal(out["shadow"][:n].view(np.int32), want.view(np.int32)) and np.all(out["shadow"][n:] == SENT)
    second = slice(4 * oo.GRID_CAP, n)
    assert not np.array_equal(out["w"][second], inp["w"][second]) and not np.array_equal(out["v"][second], inp["v"][second])


def test_opt_keras_second_trip_of_the_stride_loop(lib):
    """The same n through fn_opt_keras_ema for a two-slot rule: bit-exact against optimizer_oracle.step and ema_oracle.update."""
    name, dt, t, lr = "RMSPROP", BF, 3, 0.004
    rule = OPTIMIZERS[name]
    inp, n, n_decay, n_lp = oo.stride_inputs(), oo.STRIDE_N, oo.STRIDE_N_DECAY, oo.STRIDE_N_LP
    w, g, s1, s2, shadow = (_dev(inp[k]) for k in ("w", "g", "v", "m", "shadow"))         # rms >= 0, momentum of either sign
    wlp0 = _pattern(n + PAD)
    wlp = wlp0.cuda()
    hyper = _hyper(t, lr=lr)
    _lib.check(lib.fn_opt_keras_ema(rule.code, ptr(w), ptr(g), ptr(s1), ptr(s2), ptr(wlp), n_lp, n, n_decay, ptr(hyper), rule.rho,
                                    rule.momentum, rule.epsilon, oo.L2, dt, ptr(shadow), oo.DECAY, stream()), "opt_keras_ema")
    torch.cuda.synchronize()
    want_w, (want_s1, want_s2) = optimizer_oracle.step(name, inp["w"], inp["g"], [inp["v"], inp["m"]], lr, grad_scale=oo.GS, l2=oo.L2,
                                                       n_decay=n_decay)
    want_sh = ema_oracle.update(inp["shadow"], want_w, t, oo.DECAY)
    for got, want, what in ((w, want_w, "w"), (s1, want_s1, "rms"), (s2, want_s2, "momentum"), (shadow, want_sh, "shadow"), (g, inp["g"], "g")):
        got = got.cpu().numpy()
        assert np.array_equal(got[:n].view(np.int32), np.asarray(want, dtype=F).view(np.int32)), what
        assert np.all(got[n:] == SENT), what
    got = wlp.cpu().numpy()
    assert np.array_equal(got[:n_lp], oo.pack_rne(want_w[:n_lp], dt)) and np.array_equal(got[n_lp:], wlp0.numpy()[n_lp:])
    assert not np.array_equal(want_w[4 * oo.GRID_CAP:], inp["w"][4 * oo.GRID_CAP:])


# ---- 3. fn_adam_tick ----------------------------------------------------------------------------------------------------------
def test_adam_tick_powers_bit_for_bit(lib):
    """t = 1 .. 2048 ticked in sequence, then 10^4 and 10^5: words 1 and 2 equal adam_beta_powers(t) bit for bit, word 4 is t,
    the other words are left alone.  No exact power of the set is nearer than 7e4 fp64 ulps to an fp32 rounding tie
    (test_optim_refs_host.py), so a mismatch is a finding, not noise."""
    ts = list(range(1, 2049)) + [10 ** 4, 10 ** 5]
    rows = torch.zeros(len(ts), 8, device="cuda")
    hyper = torch.tensor([0.05, 1.0, 1.0, 0.5, 0.0, 7.0, 8.0, 9.0], device="cuda")
    for i, t in enumerate(ts):
        if t > 2048:
            hyper.view(torch.int32)[4:5].fill_(t - 1)
        _lib.check(lib.fn_adam_tick(ptr(hyper), oo.BETA1, oo.BETA2, stream()), "adam_tick")
        rows[i].copy_(hyper)
    torch.cuda.synchronize()
    got = rows.cpu().numpy()
    want = np.array([adam_beta_powers(t, oo.BETA1, oo.BETA2) for t in ts], dtype=F)
    assert np.array_equal(got.view(np.int32)[:, 4], np.array(ts, dtype=np.int32))
    bad = np.nonzero((got[:, 1:3].view(np.uint32) != want.view(np.uint32)).any(axis=1))[0]
    assert not len(bad), [(ts[i], got[i, 1:3], want[i]) for i in bad[:5]]
    assert np.all(got[:, 0] == F(0.05)) and np.all(got[:, 3] == F(0.5)) and np.all(got[:, 5:] == np.array([7.0, 8.0, 9.0], dtype=F))
    assert want[1100, 0] == 0 and 0 < want[-1, 1] < 2.0 ** -126           # beta1^1101 == 0; beta2^100000 is subnormal


# ---- 4. fn_fold_bn ------------------------------------------------------------------------------------------------------------
def _run_fold(lib, tab, total, w, beta, mean, var, max_elems, dt):
    CB = beta.size
    bufs = [torch.from_numpy(a).cuda() for a in (w, beta, mean, var)]
    tab_d = torch.from_numpy(tab).cuda()
    wf0 = _pattern(total + PAD)
    wf = wf0.cuda()
    fb = torch.full((CB + PAD,), float(SENT), device="cuda")
    _lib.check(lib.fn_fold_bn(ptr(bufs[0]), ptr(wf), ptr(fb), ptr(bufs[1]), ptr(bufs[2]), ptr(bufs[3]), ptr(tab_d), len(tab), max_elems,
                              oo.BN_EPS, dt, stream()), "fold_bn")
    torch.cuda.synchronize()
    for b, a in zip(bufs, (w, beta, mean, var)):
        assert np.array_equal(b.cpu().numpy().view(np.int32), a.view(np.int32)), "fold_bn changed an input"
    assert np.array_equal(tab_d.cpu().numpy(), tab)
    return wf.cpu().numpy(), wf0.numpy(), fb.cpu().numpy()


def _check_fold(got, wf0, fb, tab, total, w, beta, mean, var, dt, what):
    wf, bound, exact, fb_ref, fb_bound, fb_cov = oo.fold_ref(tab, total, w, beta, mean, var, dt)
    cov = oo.covered(tab, total)
    eo.check_bound(oo.lp_values(got[:total], dt)[cov], wf[cov], bound[cov], f"{what} folded weights")
    assert np.array_equal(got[:total][exact], oo.pack_rne(w, dt)[exact]), f"{what}: a layer without BatchNorm is w, rounded"
    assert np.array_equal(got[:total][~cov], wf0[:total][~cov]) and np.array_equal(got[total:], wf0[total:]), f"{what}: wrote between the layers"
    eo.check_bound(fb[:beta.size][fb_cov], fb_ref[fb_cov], fb_bound[fb_cov], f"{what} fold_bias")
    assert np.all(fb[:beta.size][~fb_cov] == SENT) and np.all(fb[beta.size:] == SENT), f"{what}: fold_bias written outside the layers' ranges"


@pytest.mark.parametrize("gx1", [False, True], ids=["real_max", "gx1"])
@pytest.mark.parametrize("dt", DTS)
def test_fold_bn_table_edges(lib, dt, gx1):
    """6 layers at offsets with gaps: 8 vectors in all, 3x3x8, ktot 1792, bn = fb = -1, bn >= 0 with fb = -1, cout 40; variances
    0 / ~1 / 1e-12 / 1e6 on adjacent channels, every third bias cancelling.  gx1: max_layer_elems = 1, one workgroup strides every
    layer."""
    tab, total, w, beta, mean, var = oo.fold_inputs(oo.FOLD_SHAPES, oo.FOLD_CB)
    max_elems = 1 if gx1 else int((tab[:, 1] * tab[:, 2]).max())
    got, wf0, fb = _run_fold(lib, tab, total, w, beta, mean, var, max_elems, dt)
    _check_fold(got, wf0, fb, tab, total, w, beta, mean, var, dt, f"dt {dt} max_layer_elems {max_elems}")


@pytest.mark.parametrize("dt", DTS)
def test_fold_bn_second_trip_of_the_stride_loop(lib, dt):
    """One layer of cout 296, ktot 1792: 530,432 elements > 256 * 2048, past the grid cap."""
    tab, total, w, beta, mean, var = oo.fold_inputs(oo.FOLD_BIG, oo.FOLD_BIG_CB)
    got, wf0, fb = _run_fold(lib, tab, total, w, beta, mean, var, int(tab[0, 1] * tab[0, 2]), dt)
    _check_fold(got, wf0, fb, tab, total, w, beta, mean, var, dt, f"dt {dt} big layer")


# ---- 5. fn_pack_transpose -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gx1", [False, True], ids=["real_max", "gx1"])
@pytest.mark.parametrize("dt", DTS)
def test_pack_transpose_table_edges(lib, dt, gx1):
    """8 layers at offsets with gaps, the 64 x 64 path (partial tiles, 7 and 9 taps, 168 tiles against a grid cap of 128) and
    the scalar path (cout 19 and 37), bit for bit; the gaps of the destination keep their sentinels.  The kernel is a 16-bit move:
    the data is the same for both dtype codes."""
    tab, total, src, sentinel = oo.transpose_inputs()
    max_elems = 1 if gx1 else int((tab[:, 1] * tab[:, 2]).max())
    w, wt, tab_d = torch.from_numpy(src).cuda(), torch.from_numpy(sentinel.copy()).cuda(), torch.from_numpy(tab).cuda()
    _lib.check(lib.fn_pack_transpose(ptr(w), ptr(wt), ptr(tab_d), len(tab), max_elems, dt, stream()), "pack_transpose")
    torch.cuda.synchronize()
    want, got = oo.transpose_ref(tab, src, sentinel), wt.cpu().numpy()
    for i, (off, cout, ktot) in enumerate(tab[:, :3]):
        sl = slice(off, off + cout * ktot)
        assert np.array_equal(got[sl], want[sl]), f"layer {i} {tuple(tab[i, [1, 3, 4]])}"
    assert np.array_equal(got, want), "wrote between the layers"
    assert np.array_equal(w.cpu().numpy(), src)


# ---- 6. rejected arguments ----------------------------------------------------------------------------------------------------
def test_adam_rejects_bad_arguments_and_writes_nothing(lib):
    n = 64
    inp = {k: np.linspace(0.5, 1.5, n).astype(F) for k in ("w", "g", "m", "v", "shadow")}
    bufs = {k: _dev(a) for k, a in inp.items()}
    before = {k: b.clone() for k, b in bufs.items()}
    wlp0 = _pattern(n + PAD)
    wlp = wlp0.cuda()
    hyper = _hyper(3)
    hyper0 = hyper.clone()

    def call(ema, n=n, n_lp=n, n_decay=n, dt=BF, null=None, shadow=True, decay=oo.DECAY):
        p = {k: (None if k == null else ptr(b)) for k, b in bufs.items()}
        args = (p["w"], p["g"], p["m"], p["v"], ptr(wlp), n_lp, n, n_decay, None if null == "hyper" else ptr(hyper), oo.BETA1, oo.BETA2,
                oo.EPS, oo.L2, dt)
        if ema:
            return lib.fn_adam_keras_ema(*args, p["shadow"] if shadow else None, decay, stream())
        return lib.fn_adam_keras(*args, stream())

    bad = [dict(n_lp=-4), dict(n_lp=-1), dict(n_lp=n + 4), dict(n_lp=6), dict(n=62, n_lp=60, n_decay=60), dict(n=0, n_lp=0, n_decay=0),
           dict(n_decay=-1), dict(n_decay=n + 1), dict(dt=7), dict(null="w"), dict(null="g"), dict(null="m"), dict(null="v"), dict(null="hyper")]
    for ema in (False, True):
        for kw in bad:
            assert call(ema, **kw) == FN_EINVAL, (ema, kw)
            with pytest.raises(ValueError):
                _lib.check(call(ema, **kw), "adam_keras")
    for kw in (dict(shadow=False), dict(decay=1.0), dict(decay=0.0)):
        assert call(True, **kw) == FN_EINVAL, kw
    torch.cuda.synchronize()
    for k, b in bufs.items():
        assert torch.equal(b, before[k]), k
    assert torch.equal(wlp.cpu(), wlp0) and torch.equal(hyper, hyper0)
    assert call(False, n_lp=0) == 0 and call(True, n_lp=0) == 0             # n_lp = 0 is the smallest valid pack
    torch.cuda.synchronize()
    assert torch.equal(wlp.cpu(), wlp0) and not torch.equal(bufs["w"], before["w"])


def test_fold_bn_rejects_bad_arguments_and_writes_nothing(lib):
    tab, total, w, beta, mean, var = oo.fold_inputs(oo.FOLD_SHAPES[:2], oo.FOLD_CB)
    bufs = [torch.from_numpy(a).cuda() for a in (w, beta, mean, var)]
    tab_d = torch.from_numpy(tab).cuda()
    wf0 = _pattern(total)
    wf = wf0.cuda()
    fb = torch.full((oo.FOLD_CB,), float(SENT), device="cuda")
    good = int((tab[:, 1] * tab[:, 2]).max())

    def call(max_elems=good, n_layers=len(tab), dt=HF, null=None):
        p = [None if null == i else ptr(b) for i, b in enumerate([bufs[0], wf, fb, bufs[1], bufs[2], bufs[3], tab_d])]
        return lib.fn_fold_bn(*p, n_layers, max_elems, oo.BN_EPS, dt, stream())

    bad = [dict(max_elems=0), dict(max_elems=-1), dict(max_elems=-(1 << 20)), dict(n_layers=0), dict(n_layers=-1), dict(dt=2)]
    bad += [dict(null=i) for i in range(7)]
    for kw in bad:
        assert call(**kw) == FN_EINVAL, kw
        with pytest.raises(ValueError):
            _lib.check(call(**kw), "fold_bn")
    torch.cuda.synchronize()
    assert torch.equal(wf.cpu(), wf0) and bool((fb == float(SENT)).all())
    for b, a in zip(bufs, (w, beta, mean, var)):
        assert np.array_equal(b.cpu().numpy(), a)
    assert call() == 0
    torch.cuda.synchronize()
    assert not torch.equal(wf.cpu(), wf0)
