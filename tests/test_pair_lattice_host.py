"""The inputs and the allowance of the exact-count GPU tests, proven on the CPU (tests/pair_lattice.py):
lattice dots are exact in the kernels' fp32 chain, the integer oracle equals the restated reference, and on the random pools the
fp32 chain stays inside the bound, flips only ambiguous incidences, and the ambiguous share stays under the cap."""
import functools

import numpy as np
import pytest

from oracle import statistics_oracle as so
from tests import pair_lattice as pl
from tests import validation_folds_oracle as vo

# (E0, E_pad, scale): the five forms the GPU tests use
FORMS = [(64, 3, 1.0), (16, 4, 1.0), (16, 20, 1.0), (4, 0, 1.0), (64, 0, 1 + 2.0 ** -5)]


@pytest.mark.parametrize("E0,E_pad,scale", FORMS)
def test_lattice_dots_are_exact_in_the_fp32_chain(E0, E_pad, scale):
    emb, starts, H = pl.lattice_classes([1, 2, 9, 33], seed=3, flips=E0 // 2, E_pad=E_pad, scale=scale, E0=E0)
    assert emb.shape == (45, E0 + E_pad) and emb.dtype == np.float32
    want = emb.astype(np.float64) @ emb.astype(np.float64).T
    got = pl.fp32_chain(emb, emb)
    assert np.array_equal(got.astype(np.float64), want)                       # bit for bit: nothing was rounded
    assert np.array_equal(want, pl.exact_dots(H, E0, scale))
    # descending order gives the same bits: exact in any summation order
    assert np.array_equal(pl.fp32_chain(emb[:, ::-1], emb[:, ::-1]), got)
    assert np.array_equal(np.linalg.norm(emb.astype(np.float64), axis=1), np.full(45, float(np.float32(scale))))
    # the planted pairs of the 9-row class: duplicate, negated, orthogonal
    r = int(starts[2])
    assert H[r, r + 1] == 0 and H[r, r + 2] == E0 and H[r, r + 3] == E0 // 2
    if scale != 1.0:
        assert want.max() == 1.0634765625 and want.min() == -1.0634765625


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("E0,E_pad", [(64, 0), (16, 4)])
def test_exact_counts_equal_the_restated_reference(E0, E_pad, metric):
    sizes = [1, 2, 31, 33, 5, 1, 12]
    emb, starts, H = pl.lattice_classes(sizes, seed=11, flips=E0 // 2, E_pad=E_pad, E0=E0)
    thr = pl.lattice_thresholds(metric, E0)
    counts, P = pl.exact_counts(H, starts, thr, metric, E0)
    got, terms, wmax = pl.weighted_tables(counts, P, len(sizes))
    labels = np.repeat(np.arange(len(sizes)), sizes)
    ref = so.ConfidenceMatrix(so.SimilarityCalculator(emb.astype(np.float64), labels, metric), thr.astype(np.float64))
    for r, name in enumerate(pl.ROWS):
        want = getattr(ref, name)
        assert np.all(np.abs(got[r] - want) <= terms[r] * 2.0 ** -52 * want), name
    assert terms[0] == 5 and terms[2] == 21 and wmax == 33 * 31 * 21.0        # two one-row classes have no diagonal pair
    assert np.all(got[0, 0] == 0) and np.all(got[2, 0] == 0)                  # threshold 0 counts nothing, duplicates included
    assert got[3, -1] == 0 and got[1, -1] == 0                                # the topmost threshold counts every pair
    if metric == 0:                                                           # on a threshold is not below it
        n = int(np.flatnonzero(thr == 2.0)[0])
        a, b, slot = pl._pairs(starts)
        on = np.bincount(slot[4 * H[a, b] == 2 * E0], minlength=len(P))
        assert on.sum() >= 3 and np.array_equal(counts[:, n + 1] - counts[:, n], on)


@pytest.mark.parametrize("metric", [0, 1])
def test_fold_variant_equals_the_one_pass_restatement(metric):
    sizes = [1, 2, 1, 5, 9, 2, 1, 3, 30, 1]
    F = 4
    emb, starts, H = pl.lattice_classes(sizes, seed=7, flips=20)
    rng = np.random.default_rng(0)
    fold = rng.integers(0, F, len(emb))
    fold[starts[1]:starts[2]] = 2                                             # a class whose rows are all held out in one fold
    thr = pl.lattice_thresholds(metric)
    counts, _ = pl.exact_counts(H, starts, thr, metric, fold=fold, F=F)
    got, terms, _ = pl.weighted_tables_folds(counts, starts, fold, F)
    labels = np.repeat(np.arange(len(sizes)), sizes)
    want, cells = vo.onepass(emb, labels, fold, thr.astype(np.float64), F, metric)
    assert cells >= 1
    assert np.all(np.abs(got - want) <= terms[:, :, None] * 2.0 ** -52 * want)
    rows, classes = pl.train_tables(starts, fold, F)
    ref_rows, ref_classes = vo.tables(labels, fold, F)
    assert np.array_equal(rows, ref_rows) and np.array_equal(classes, ref_classes)


@functools.lru_cache(maxsize=None)
def _chain(sizes, E):
    emb, starts, _ = pl.sorted_pool(list(sizes), E)
    return emb, starts, pl.fp32_chain(emb, emb)


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("sizes,E", pl.RANDOM_POOLS)
def test_random_pools_flip_only_ambiguous_incidences_and_keep_the_cap(sizes, E, metric):
    emb, starts, s32 = _chain(tuple(sizes), E)
    s64, delta = pl.dot_bound(emb)
    assert np.all(np.abs(s32.astype(np.float64) - s64) <= delta)              # the fp32 chain stays within gamma_E sum |a b|
    thr = pl.random_thresholds(metric)
    a, b, slot, amb = pl.ambiguous_mask(emb, starts, thr, metric)
    t64 = thr.astype(np.float64)[None, :]
    below32 = pl.distance32(s32[a, b], metric)[:, None] < thr[None, :]
    below64 = pl.distance64(s64[a, b], metric)[:, None] < t64
    flips = below32 != below64
    share = amb.sum() / len(a)
    print(sizes[:4], E, "metric", metric, "pairs", len(a), "ambiguous incidences", int(amb.sum()), "share %.4f %%" % (100 * share),
          "flips of the emulated chain", int(flips.sum()))
    assert not np.any(flips & ~amb)                                           # every flip is an ambiguous incidence
    assert share <= pl.CAP
    assert np.array_equal(pl.ambiguity(emb, starts, thr, metric).sum(), amb.sum())
    # the tables of the emulated chain stay within the allowance the GPU test grants
    C = len(sizes)
    counts, P = pl.counts64(emb, starts, thr, metric)
    want, terms, _ = pl.weighted_tables(counts, P, C)
    h = np.zeros((len(P), len(thr)), np.int64)
    np.add.at(h, slot, below32.astype(np.int64))
    got, _, _ = pl.weighted_tables(h, P, C)
    allow = pl.allowance(pl.ambiguity(emb, starts, thr, metric), P, C)
    assert np.all(np.abs(got - want) <= allow + terms[:, None] * 2.0 ** -52 * want)
