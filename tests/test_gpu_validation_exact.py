"""fn_confidence_counts and fn_confidence_counts_folds held to exact counts ("Exact counts").

Lattice rows (tests/pair_lattice.py) have dot products that are exact in fp32 in any order, so the device and the integer oracle
must agree on every count: the only allowance is the reordering of the fp64 additions, n_terms 2^-52 relative, and every test shows
that one miscounted pair (1 / the largest weight) is more than 1000 times that.  Random unit rows are compared with fp64 under the
proven ambiguity allowance, after its cap has been asserted.  Every launch goes through the C ABI with guard words behind `out` and
`range`; `range` is compared by value."""
import functools

import numpy as np
import pytest
import torch

from facenet_amd import _lib
from facenet_amd.statistics import _decode_ord
from tests import pair_lattice as pl

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 8
FILL_D, FILL_I = -77.0, -77


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _finish(out, rng, n_out):
    torch.cuda.synchronize()
    o, r = out.cpu().numpy(), rng.cpu().tolist()
    assert (o[n_out:] == FILL_D).all() and r[2:] == [FILL_I] * GUARD              # nothing behind out and range was touched
    lo, hi = _decode_ord(r[0]), _decode_ord(r[1])
    return o[:n_out], ((lo, hi) if hi >= lo else None)


def run_base(emb, starts, thr, metric):
    """fn_confidence_counts -> (table [4, T], (min, max) of the dots or None when no pair was evaluated)."""
    lib = _lib.load()
    T, C = len(thr), len(starts) - 1
    e, s, t = _dev(emb, np.float32), _dev(starts, np.int32), _dev(thr, np.float32)
    out = torch.full((4 * T + GUARD,), FILL_D, dtype=torch.float64, device=DEV)
    rng = torch.full((2 + GUARD,), FILL_I, dtype=torch.int32, device=DEV)
    rc = lib.fn_confidence_counts(e.data_ptr(), s.data_ptr(), C, emb.shape[1], t.data_ptr(), T, metric, out.data_ptr(), rng.data_ptr(), _stream())
    assert rc == 0, lib.fn_last_error()
    o, r = _finish(out, rng, 4 * T)
    return o.reshape(4, T), r


def run_folds(emb, starts, fold, F, thr, metric):
    """fn_confidence_counts_folds -> (tables [F, 4, T], range)."""
    lib = _lib.load()
    T, C = len(thr), len(starts) - 1
    rows, classes = pl.train_tables(starts, fold, F)
    e, s, t = _dev(emb, np.float32), _dev(starts, np.int32), _dev(thr, np.float32)
    fd, rd, cd = _dev(fold, np.int32), _dev(rows, np.int32), _dev(classes, np.int32)
    out = torch.full((F * 4 * T + GUARD,), FILL_D, dtype=torch.float64, device=DEV)
    rng = torch.full((2 + GUARD,), FILL_I, dtype=torch.int32, device=DEV)
    rc = lib.fn_confidence_counts_folds(e.data_ptr(), s.data_ptr(), fd.data_ptr(), rd.data_ptr(), cd.data_ptr(), C, emb.shape[1], F, t.data_ptr(),
                                        T, metric, out.data_ptr(), rng.data_ptr(), _stream())
    assert rc == 0, lib.fn_last_error()
    o, r = _finish(out, rng, F * 4 * T)
    return o.reshape(F, 4, T), r


def assert_exact(got, want, terms, wmax, what):
    """|got - want| <= n_terms 2^-52 want per entry, and one miscounted pair is more than 1000 times the largest such bound."""
    bound = terms[..., None] * 2.0 ** -52 * want
    assert 1.0 / wmax > 1000 * bound.max(), (what, wmax, bound.max())
    err = np.abs(got - want)
    bad = ~(err <= bound)
    if bad.any():
        idx = tuple(int(v) for v in np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} entries differ; first at {idx}: got {got[idx]!r}, want {want[idx]!r}, "
                             f"one pair is worth at least {1.0 / wmax:.3g}")


def check_base(emb, starts, H, thr, metric, E0=64, scale=1.0, what=""):
    counts, P = pl.exact_counts(H, starts, thr, metric, E0, scale)
    want, terms, wmax = pl.weighted_tables(counts, P, len(starts) - 1)
    got, rng = run_base(emb, starts, thr, metric)
    assert_exact(got, want, terms, wmax, f"confidence_counts {what} metric {metric}")
    assert rng == pl.want_range(pl.exact_dots(H, E0, scale), starts), what
    return got, want


def check_folds(emb, starts, H, fold, F, thr, metric, E0=64, scale=1.0, what=""):
    counts, _ = pl.exact_counts(H, starts, thr, metric, E0, scale, fold=fold, F=F)
    want, terms, wmax = pl.weighted_tables_folds(counts, starts, fold, F)
    got, rng = run_folds(emb, starts, fold, F, thr, metric)
    assert_exact(got, want, terms, wmax, f"confidence_counts_folds {what} metric {metric} F {F}")
    assert rng == pl.want_range(pl.exact_dots(H, E0, scale), starts, fold, F), what
    return got, want


def _folds(n, F, seed):
    return np.random.default_rng(seed).integers(0, F, n)


# ---- a. tile edges -------------------------------------------------------------------------------------------------------------
TILE_SIZES = [1, 2, 31, 32, 33, 63, 64, 65, 129]      # around the 32-row tile of confidence_kernel and the 64-row super-tile


@functools.lru_cache(maxsize=None)
def tile_case():
    return pl.lattice_classes(TILE_SIZES, seed=1, flips=32)


@pytest.mark.parametrize("metric", [0, 1])
def test_tile_edges_base_kernel(metric):
    emb, starts, H = tile_case()
    thr = pl.lattice_thresholds(metric)
    assert len(thr) == 66 and thr[0] == 0
    got, want = check_base(emb, starts, H, thr, metric, what="tile edges")
    assert np.all(got[0, 0] == 0) and np.all(got[2, 0] == 0)                       # threshold 0 counts nothing, duplicate rows included
    assert got[3, -1] == 0 and got[1, -1] == 0 and got[0, -1] > 0 and got[2, -1] > 0           # the topmost counts every pair


@pytest.mark.parametrize("F", [2, 3])
@pytest.mark.parametrize("metric", [0, 1])
def test_tile_edges_fold_kernel(metric, F):
    emb, starts, H = tile_case()
    thr = pl.lattice_thresholds(metric)
    got, _ = check_folds(emb, starts, H, _folds(len(emb), F, 5), F, thr, metric, what="tile edges")
    assert np.all(got[:, 0, 0] == 0) and np.all(got[:, 2, 0] == 0) and np.all(got[:, 3, -1] == 0) and np.all(got[:, 1, -1] == 0)


# ---- b. E edges ----------------------------------------------------------------------------------------------------------------
# (E0, E_pad): E = 64, 67 (the fold kernel's scalar staging path, the base kernel's partial 64-chunk), 20 and 4
@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("E0,E_pad", [(64, 0), (64, 3), (16, 4), (4, 0)])
def test_embedding_size_edges(E0, E_pad, metric):
    emb, starts, H = pl.lattice_classes([1, 2, 33, 5, 65], seed=2, flips=E0 // 2, E_pad=E_pad, E0=E0)
    assert emb.shape[1] == E0 + E_pad
    thr = pl.lattice_thresholds(metric, E0)
    check_base(emb, starts, H, thr, metric, E0, what=f"E {E0 + E_pad}")
    check_folds(emb, starts, H, _folds(len(emb), 3, 6), 3, thr, metric, E0, what=f"E {E0 + E_pad}")


# ---- c. T edges ----------------------------------------------------------------------------------------------------------------
def _threshold_run(T, seed):
    """T ascending thresholds from the attainable distances (multiples of 1/16 in [0, 4]) with runs of equal values, a leading block
    below every distance (<= 0) and a trailing block above every distance (> 4)."""
    rng = np.random.default_rng(seed)
    lead, trail = T // 8, T // 8
    mid = np.sort(rng.integers(0, 65, T - lead - trail)) / 16.0
    thr = np.concatenate([np.linspace(-1, 0, lead), mid, np.linspace(4.25, 6, trail)]).astype(np.float32)
    assert len(thr) == T and np.all(np.diff(thr) >= 0)
    return thr


@pytest.mark.parametrize("T", [1, 2, 63, 64, 65, 128, 129, 256])
def test_threshold_count_edges(T):
    """The fold kernel's wave prefix scan carries across 64-lane chunks; the base kernel's prefix is serial."""
    emb, starts, H = pl.lattice_classes([3, 40, 1, 70], seed=3, flips=32)
    thr = _threshold_run(T, T)
    if T >= 63:
        assert np.any(np.diff(thr) == 0)
    base, _ = check_base(emb, starts, H, thr, 0, what=f"T {T}")
    folds, _ = check_folds(emb, starts, H, _folds(len(emb), 3, 7), 3, thr, 0, what=f"T {T}")
    same = np.flatnonzero(np.diff(thr) == 0)
    lead, trail = T // 8, T // 8
    for tab in (base, *folds):
        # equal thresholds hold equal counts: the sums differ at most by the order of their additions
        assert np.all(np.abs(tab[:, same] - tab[:, same + 1]) <= 12 * 2.0 ** -52 * tab[:, same])
        assert np.all(tab[0, :lead] == 0) and np.all(tab[2, :lead] == 0)
        assert np.all(tab[3, T - trail:] == 0) and np.all(tab[1, T - trail:] == 0)


# ---- d. clamp and range ----------------------------------------------------------------------------------------------------------
SCALE = 1 + 2.0 ** -5


def _attainable_thresholds(metric, E0, scale):
    d = np.unique(pl.distance64(pl.exact_dots(np.arange(E0 + 1), E0, scale), metric))
    if metric == 0:
        return np.concatenate([d, [4.5]]).astype(np.float32)                       # exact in fp32: on every attainable distance
    return np.concatenate([[0.0], (d[:-1] + d[1:]) / 2, [3.2]]).astype(np.float32)


@pytest.mark.parametrize("metric", [0, 1])
def test_clamp_and_range_on_scaled_rows(metric):
    emb, starts, H = pl.lattice_classes([5, 33, 2, 70], seed=4, flips=32, scale=SCALE)
    dots = pl.exact_dots(H, 64, SCALE)
    assert pl.want_range(dots, starts) == (-1.0634765625, 1.0634765625)            # the duplicate and the negated rows
    thr = _attainable_thresholds(metric, 64, SCALE)
    assert thr[0] == 0 and (metric == 1 or np.isin(np.unique(pl.distance64(dots, 0)), thr.astype(np.float64)).all())
    got, _ = check_base(emb, starts, H, thr, metric, scale=SCALE, what="scaled")
    # s > 1 lands in the d = 0 bin: not counted at threshold 0, counted at the next one
    assert got[0, 0] == 0 and got[0, 1] > 0
    for F in (2, 3):
        check_folds(emb, starts, H, _folds(len(emb), F, 8), F, thr, metric, scale=SCALE, what="scaled")


@pytest.mark.parametrize("scale", [1.0, SCALE])
def test_fold_kernel_range_rule(scale):
    """Classes of two identical rows held out in different folds: with F = 2 such a pair is in no training part and `range` must not
    reach its dot product; with F = 3 (fold 2 holds nothing out) it is in the third part and `range` must reach it."""
    emb, starts, H = pl.lattice_classes([2, 2, 2, 1, 2], seed=9, flips=20, scale=scale)
    fold = np.array([0, 1, 0, 1, 0, 1, 1, 0, 1])
    dots = pl.exact_dots(H, 64, scale)
    top = float(np.float32(scale)) ** 2
    thr = pl.lattice_thresholds(0)
    lo2, hi2 = pl.want_range(dots, starts, fold, 2)
    assert pl.want_range(dots, starts)[1] == top and hi2 < top
    _, rng2 = run_folds(emb, starts, fold, 2, thr, 0)
    assert rng2 == (lo2, hi2)
    _, rng3 = run_folds(emb, starts, fold, 3, thr, 0)
    assert rng3 == pl.want_range(dots, starts) and rng3[1] == top
    check_folds(emb, starts, H, fold, 2, thr, 0, scale=scale, what="straddling duplicates")
    check_folds(emb, starts, H, fold, 3, thr, 0, scale=scale, what="straddling duplicates")
    _, rng = run_base(emb, starts, thr, 0)
    assert rng == pl.want_range(dots, starts)


# ---- e. many class pairs per workgroup -----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def many_classes():
    """300 classes of sizes cycling 1, 2, 3, 5; the cycle shifts by one from class 256 on, so that a diagonal workgroup (stride 256)
    meets a one-row class and then a populated one, or the reverse.  44 850 off-diagonal class pairs over 2048 workgroups.  Folds by
    hand: a one-row class has no training row in its fold; every 8th class is held out whole in one fold."""
    F = 4
    sizes, emb, starts, H = pl.many_class_pool()
    cls = pl._class_of(starts)
    fold = (cls + np.arange(len(cls)) - starts[cls]) % F                            # class c, position p: fold (c + p) % 4
    whole = cls % 8 == 5
    fold[whole] = (cls[whole] // 8) % F
    rows, _ = pl.train_tables(starts, fold, F)
    assert sizes[0] == 1 and sizes[256] == 2 and sizes[3] == 5 and sizes[259] == 1
    assert (rows == 0).sum() >= 75 + 30 and emb.shape == (sum(sizes), 20)
    thr = (np.arange(33) / 8.0).astype(np.float32)                                  # on every attainable distance h / 4
    return emb, starts, H, fold, F, thr


def test_many_class_pairs_per_workgroup():
    emb, starts, H, fold, F, thr = many_classes()
    got, _ = check_folds(emb, starts, H, fold, F, thr, 0, E0=16, what="300 classes")
    check_base(emb, starts, H, thr, 0, E0=16, what="300 classes")
    # against fn_confidence_counts on each training part
    for f in range(F):
        keep = fold != f
        left = np.add.reduceat(keep.astype(np.int64), starts[:-1])
        sub = np.concatenate([[0], np.cumsum(left[left > 0])])
        ref, _ = run_base(emb[keep], sub, thr, 0)
        C = len(sub) - 1
        assert np.all(np.abs(got[f] - ref) <= C * (C + 1) / 2 * 2.0 ** -52 * np.abs(ref)), f


@pytest.mark.parametrize("metric", [0, 1])
def test_single_class(metric):
    """C = 1: the fold kernel launches no off-diagonal workgroup, fp and tn stay zero."""
    emb, starts, H = pl.lattice_classes([70], seed=13, flips=32)
    thr = pl.lattice_thresholds(metric)
    got, _ = check_base(emb, starts, H, thr, metric, what="one class")
    assert np.all(got[1] == 0) and np.all(got[2] == 0)
    folds, _ = check_folds(emb, starts, H, _folds(70, 3, 14), 3, thr, metric, what="one class")
    assert np.all(folds[:, 1] == 0) and np.all(folds[:, 2] == 0)


# ---- f. random unit rows under the proven allowance -------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def random_case(sizes, E, metric):
    emb, starts, _ = pl.sorted_pool(list(sizes), E)
    thr = pl.random_thresholds(metric)
    return emb, starts, thr


def _assert_within_allowance(got, want, terms, allow, what):
    bound = allow + terms[:, None] * 2.0 ** -52 * want
    err = np.abs(got - want)
    print(what, "largest allowance", float(allow.max()), "largest difference", float(err.max()))
    bad = ~(err <= bound)
    assert not bad.any(), (what, [tuple(int(v) for v in i) for i in np.argwhere(bad)[:4]], float((err - bound).max()))


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("sizes,E", pl.RANDOM_POOLS)
def test_random_rows_base_kernel(sizes, E, metric):
    emb, starts, thr = random_case(tuple(sizes), E, metric)
    C = len(sizes)
    amb = pl.ambiguity(emb, starts, thr, metric)
    counts, P = pl.counts64(emb, starts, thr, metric)
    share = amb.sum() / P.sum()
    print(sizes[:4], E, "metric", metric, "pairs", int(P.sum()), "ambiguous incidences", int(amb.sum()), "share %.4f %%" % (100 * share))
    assert share <= pl.CAP                                                         # a condition on the case, before any device output
    want, terms, _ = pl.weighted_tables(counts, P, C)
    got, rng = run_base(emb, starts, thr, metric)
    _assert_within_allowance(got, want, terms, pl.allowance(amb, P, C), f"confidence_counts {sizes[:4]} E {E} metric {metric}")
    s64, delta = pl.dot_bound(emb)
    a, b, _ = pl._pairs(starts)
    assert s64[a, b].min() - delta.max() <= rng[0] <= s64[a, b].min() + delta.max()
    assert s64[a, b].max() - delta.max() <= rng[1] <= s64[a, b].max() + delta.max()


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("sizes,E", pl.RANDOM_POOLS)
def test_random_rows_fold_kernel(sizes, E, metric):
    emb, starts, thr = random_case(tuple(sizes), E, metric)
    F = 3
    fold = _folds(len(emb), F, len(sizes))
    amb_all = pl.ambiguity(emb, starts, thr, metric)
    _, P_all = pl.counts64(emb, starts, thr, metric)
    share = amb_all.sum() / P_all.sum()
    print(sizes[:4], E, "metric", metric, "pairs", int(P_all.sum()), "ambiguous incidences", int(amb_all.sum()), "share %.4f %%" % (100 * share))
    assert share <= pl.CAP
    amb = pl.ambiguity(emb, starts, thr, metric, fold, F)
    counts, _ = pl.counts64(emb, starts, thr, metric, fold, F)
    want, terms, _ = pl.weighted_tables_folds(counts, starts, fold, F)
    got, _ = run_folds(emb, starts, fold, F, thr, metric)
    for f, (P, Cf) in enumerate(pl.fold_weights(starts, fold, F)):
        _assert_within_allowance(got[f], want[f], terms[f], pl.allowance(amb[f], P, len(sizes), Cf),
                                 f"confidence_counts_folds {sizes[:4]} E {E} metric {metric} fold {f}")
