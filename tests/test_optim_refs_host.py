"""The references and bounds of tests/optim_oracle.py checked against each other, without a GPU: on the inputs of the GPU cases
(test_gpu_optim_edges.py) a correctly rounded fp32 restatement of Adam and of the BatchNorm fold stays inside each bound, the
references' no-underflow assertions hold, and planted errors -- an L2 boundary off by one element, eps inside the square root, no
bias correction, an unsquared gradient, a truncating pack, a neighbouring channel's scale, a missing eps, a wrong sign, a transpose
with tap and cin swapped -- fall outside.  It also re-derives, in exact rational arithmetic, how far the beta powers fn_adam_tick
rounds to fp32 stay from a rounding tie, and checks the preconditions of the 16-byte paths on the layer tables the package builds."""
import numpy as np
import pytest

from tests import elementwise_oracle as eo
from tests import optim_oracle as oo

BF, HF = eo.BF, eo.HF


def _inside(got, ref, bound):
    return bool(np.all(np.abs(np.asarray(got, dtype=np.float64) - ref) <= bound))


def _check(got, ref, bound, what):
    eo.check_bound(np.asarray(got, dtype=np.float64), ref, bound, what)


def _adam_all_inside(got, ref):
    w, m, v = got
    return _inside(m, ref["m"], ref["e_m"]) and _inside(v, ref["v"], ref["e_v"]) and _inside(w, ref["w"], ref["e_w"])


# ---- Adam -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", oo.ADAM_TS)
def test_adam_restatement_inside_bounds(t):
    inp = oo.adam_inputs()
    hyper = oo.hyper_words(t)
    if t == 1101:
        assert hyper[1] == 0
    if t == 100_000:
        assert 0 < hyper[2] < 2.0 ** -126                            # an fp32 subnormal
    if t == 10 ** 6:
        assert hyper[1] == 0 and hyper[2] == 0
    for n_decay in oo.ADAM_N_DECAY:
        ref = oo.adam_ref(inp["w"], inp["g"], inp["m"], inp["v"], hyper, n_decay)      # asserts no underflow
        w, m, v = oo.adam_f32(inp["w"], inp["g"], inp["m"], inp["v"], hyper, n_decay)
        _check(m, ref["m"], ref["e_m"], f"t {t} n_decay {n_decay} m")
        _check(v, ref["v"], ref["e_v"], f"t {t} n_decay {n_decay} v")
        _check(w, ref["w"], ref["e_w"], f"t {t} n_decay {n_decay} w")
        for lo, hi in oo.ADAM_ZERO_SEGS:                              # the zero segments stay bitwise +0
            for a in (w, m, v):
                assert not a[lo:hi].view(np.int32).any()
            assert not ref["w"][lo:hi].any() and not ref["e_w"][lo:hi].any() and not ref["e_m"][lo:hi].any() and not ref["e_v"][lo:hi].any()
        if n_decay <= oo.ADAM_TIES:                                   # undecayed, g = m = 0: the tie values reach the pack as they are
            sl = slice(oo.ADAM_TIES, oo.ADAM_TIES + inp["n_ties"])
            assert np.array_equal(w[sl].view(np.int32), inp["w"][sl].view(np.int32))


def test_adam_stride_case_restatement_inside_bounds():
    inp = oo.stride_inputs()
    assert inp["w"].size == oo.STRIDE_N > 4 * oo.GRID_CAP and oo.STRIDE_N_DECAY % 4 == 1
    assert 4 * oo.GRID_CAP < oo.STRIDE_N_DECAY < oo.STRIDE_N_LP < oo.STRIDE_N and oo.STRIDE_N_LP % 4 == 0
    hyper = oo.hyper_words(3)
    ref = oo.adam_ref(inp["w"], inp["g"], inp["m"], inp["v"], hyper, oo.STRIDE_N_DECAY)
    w, m, v = oo.adam_f32(inp["w"], inp["g"], inp["m"], inp["v"], hyper, oo.STRIDE_N_DECAY)
    _check(m, ref["m"], ref["e_m"], "m")
    _check(v, ref["v"], ref["e_v"], "v")
    _check(w, ref["w"], ref["e_w"], "w")
    # a second trip that is skipped leaves the inputs in place: far outside
    w_bad = w.copy()
    w_bad[4 * oo.GRID_CAP:] = inp["w"][4 * oo.GRID_CAP:]
    assert not _inside(w_bad, ref["w"], ref["e_w"])


def test_adam_planted_errors_fall_outside():
    inp = oo.adam_inputs()
    args = (inp["w"], inp["g"], inp["m"], inp["v"])
    n_decay = oo.ADAM_N_DECAY[2]
    for t in (1, 2, 1000):
        hyper = oo.hyper_words(t)
        ref = oo.adam_ref(*args, hyper, n_decay)
        assert _adam_all_inside(oo.adam_f32(*args, hyper, n_decay), ref)
        for off in (-1, 1):                                           # the L2 boundary off by one element, either way
            got = oo.adam_f32(*args, hyper, n_decay + off)
            assert not _inside(got[1], ref["m"], ref["e_m"]) and not _inside(got[2], ref["v"], ref["e_v"]), (t, off)
            assert not _inside(got[0], ref["w"], ref["e_w"]), (t, off)
        assert not _inside(oo.adam_f32(*args, hyper, n_decay, eps_inside_sqrt=True)[0], ref["w"], ref["e_w"]), t
        assert not _inside(oo.adam_f32(*args, hyper, n_decay, square_g=False)[2], ref["v"], ref["e_v"]), t
    hyper = oo.hyper_words(2)
    ref = oo.adam_ref(*args, hyper, n_decay)
    assert not _inside(oo.adam_f32(*args, hyper, n_decay, bias_correction=False)[0], ref["w"], ref["e_w"])


@pytest.mark.parametrize("dt", [BF, HF])
def test_truncating_pack_differs_from_round_to_nearest_even(dt):
    inp = oo.adam_inputs()
    w = oo.adam_f32(inp["w"], inp["g"], inp["m"], inp["v"], oo.hyper_words(2), 0)[0]
    rne, trunc = oo.pack_rne(w, dt), oo.pack_truncate(w, dt)
    sl = slice(oo.ADAM_TIES, oo.ADAM_TIES + inp["n_ties"])
    assert not np.array_equal(rne, trunc) and not np.array_equal(rne[sl], trunc[sl])
    # the ties are there: values exactly half way between two neighbours of the storage type, with either parity below them
    v64 = w[sl].astype(np.float64)
    lo, hi = oo.lp_values(trunc[sl], dt), oo.lp_values(trunc[sl] + 1, dt)
    tie = (np.abs(v64) - np.abs(lo) == np.abs(hi) - np.abs(v64)) & np.isfinite(hi)
    assert tie.sum() >= 64 and {0, 1} == set((trunc[sl][tie] & 1).tolist())
    assert np.array_equal(rne[sl][tie] & 1, np.zeros(int(tie.sum()), dtype=np.int16))             # ties go to the even neighbour
    if dt == HF:
        assert (np.abs(v64) < 2.0 ** -14).sum() >= 64                                              # the f16 subnormal range


def test_adam_tick_powers_stay_clear_of_fp32_rounding_ties():
    """fn_adam_tick rounds a double pow to fp32.  A pow good to 16 ulps (the OpenCL bound for double pow; libm and the device
    library do far better) rounds like the exact power as long as the exact power is further than that from an fp32 tie."""
    ts = range(1, 2049)
    d1, d2 = oo.min_tie_distance(oo.BETA1, ts), oo.min_tie_distance(oo.BETA2, ts)
    print(f"smallest distance from an fp32 rounding tie, in fp64 ulps: beta1 {d1:.3g}, beta2 {d2:.3g}")
    assert d1 > 16 and d2 > 16
    from facenet_amd.optimizers import adam_beta_powers
    b1, b2 = np.float64(np.float32(oo.BETA1)), np.float64(np.float32(oo.BETA2))
    for t in (1, 2, 970, 1101, 2048):                                # the host mirror is that double pow, rounded once
        assert adam_beta_powers(t, oo.BETA1, oo.BETA2) == (float(np.float32(b1 ** t)), float(np.float32(b2 ** t)))


# ---- fn_fold_bn ---------------------------------------------------------------------------------------------------------------
FOLD_TABLES = [("table", oo.FOLD_SHAPES, oo.FOLD_CB), ("big_layer", oo.FOLD_BIG, oo.FOLD_BIG_CB)]


def test_rsqrt_slack_comes_from_the_restatement_error():
    worst = 0.0
    for _, shapes, CB in FOLD_TABLES:
        tab, total, w, beta, mean, var = oo.fold_inputs(shapes, CB)
        t32 = var + np.float32(oo.BN_EPS)
        worst = max(worst, float(eo.ulps(eo._rsqrt32(t32), t32.astype(np.float64) ** -0.5).max()))
    print("fp32 restatement error of 1/sqrt in ulps:", worst)
    assert 0 < worst <= 0.5001
    assert eo.C_RSQRT == max(4, int(np.ceil(4 * worst)))


@pytest.mark.parametrize("dt", [BF, HF])
@pytest.mark.parametrize("name,shapes,CB", FOLD_TABLES, ids=[t[0] for t in FOLD_TABLES])
def test_fold_restatement_inside_bounds_and_planted_errors_outside(name, shapes, CB, dt):
    tab, total, w, beta, mean, var = oo.fold_inputs(shapes, CB)
    assert all(off % 8 == 0 and off > 0 for off in tab[:, 0]) and not len(oo.table_preconditions(tab))
    wf, bound, exact, fb, fb_bound, fb_cov = oo.fold_ref(tab, total, w, beta, mean, var, dt)        # asserts no underflow
    cov = oo.covered(tab, total)
    bits, bias = oo.fold_f32(tab, total, w, beta, mean, var, dt)
    _check(oo.lp_values(bits, dt)[cov], wf[cov], bound[cov], f"{name} folded weights")
    assert np.array_equal(bits[exact], oo.pack_rne(w, dt)[exact])
    _check(bias[fb_cov], fb[fb_cov], fb_bound[fb_cov], f"{name} fold_bias")
    # some channels do cancel to within a few ulps of beta
    absref = fb_bound[fb_cov] / oo.gamma(oo.K_FOLD_B)
    assert (np.abs(fb[fb_cov]) < 2.0 ** -20 * absref).sum() >= 4
    # planted errors
    bad, _ = oo.fold_f32(tab, total, w, beta, mean, var, dt, tail_from_next_channel=True)
    assert not _inside(oo.lp_values(bad, dt)[cov], wf[cov], bound[cov])
    bad, bad_bias = oo.fold_f32(tab, total, w, beta, mean, var, dt, with_eps=False)
    assert not _inside(oo.lp_values(bad, dt)[cov], wf[cov], bound[cov]) and not _inside(bad_bias[fb_cov], fb[fb_cov], fb_bound[fb_cov])
    _, bad_bias = oo.fold_f32(tab, total, w, beta, mean, var, dt, minus=False)
    assert not _inside(bad_bias[fb_cov], fb[fb_cov], fb_bound[fb_cov])


def test_fold_table_has_the_shapes_the_kernel_can_go_wrong_at():
    tab, total = oo.make_table(oo.FOLD_SHAPES)
    numel = tab[:, 1] * tab[:, 2]
    assert 64 in numel and 72 in tab[:, 2] and 1792 in tab[:, 2]                    # 8 vectors in all; 3x3x8; the widest ktot
    assert any(r[5] < 0 and r[6] < 0 for r in tab) and any(r[5] >= 0 and r[6] < 0 for r in tab)
    assert not oo.covered(tab, total).all() and 5 <= len(tab) <= 6
    big, _ = oo.make_table(oo.FOLD_BIG)
    assert big[0, 1] * big[0, 2] == 530_432 > 256 * 2048


# ---- fn_pack_transpose --------------------------------------------------------------------------------------------------------
def test_transpose_reference_and_planted_swap():
    tab, total, src, sentinel = oo.transpose_inputs()
    ref = oo.transpose_ref(tab, src, sentinel)
    cov = oo.covered(tab, total)
    assert np.array_equal(ref[~cov], sentinel[~cov]) and not cov.all()
    assert len(np.unique(src[:65536])) == 65536                                     # every 16-bit pattern moves
    for off, cout, ktot, taps, cin, _, _, _ in tab:
        # element (ci, tap, co) of the transposed layer is element (co, tap, ci) of the source, spot-checked at the corners
        for co, tap, ci in ((0, 0, 0), (cout - 1, taps - 1, cin - 1), (cout - 1, 0, cin // 2), (cout // 2, taps - 1, 0)):
            assert ref[off + (ci * taps + tap) * cout + co] == src[off + (co * taps + tap) * cin + ci]
    bad = oo.transpose_ref(tab, src, sentinel, swap_tap_cin=True)
    assert not np.array_equal(bad, ref)
    multi_tap = tab[:, 3] > 1
    assert multi_tap.any() and any(c % 8 for c in tab[:, 1]) and (np.ceil(tab[:, 1] / 64) * np.ceil(tab[:, 4] / 64) * tab[:, 3]).max() > 128


# ---- the tables the package builds --------------------------------------------------------------------------------------------
def _networks():
    from facenet_amd.engine import Network
    from facenet_amd.engine_v2 import NetworkV2
    for E in (128, 512):
        for ncls in (None, 19):
            yield f"v1 E{E} classes {ncls}", Network(embedding_size=E, nrof_classes=ncls, allocate=False)
    yield "v2 smallest", NetworkV2(128, config={"repeat": [1, 1, 1]}, nrof_classes=19, allocate=False)


def test_every_layer_table_meets_the_preconditions_of_the_16_byte_paths():
    """pack_transpose_kernel's 64 x 64 path loads 16 bytes along cin and stores 16 bytes along cout, fold_bn_kernel moves 8
    weights at a time and divides by ktot: every row needs w_off, cin and cout to be multiples of 8 and ktot == taps * cin.  The C
    entries cannot check it (the table is device memory)."""
    for name, net in _networks():
        tab = net.layer_table()
        assert tab.shape == (len(net.layers), 8) and tab.dtype == np.int32
        bad = oo.table_preconditions(tab)
        assert not len(bad), (name, bad)
        assert int((tab[:, 1] * tab[:, 2]).max()) == net.max_layer_elems > 0
        ends = tab[:, 0] + tab[:, 1] * tab[:, 2]
        assert np.all(tab[1:, 0] >= ends[:-1]) and int(ends[-1]) <= net.n_kernel       # no layer overlaps the next
    # and the check does see a bad row
    tab = tab.copy()
    tab[3, 4] += 4
    assert len(oo.table_preconditions(tab)) == 1
