"""Inputs whose pair distances are exact, and a proven allowance for those that are not ("Exact counts").

Lattice rows: every row is +-E0^-1/2 in its first E0 columns (E0 = 4, 16 or 64, so the value is a power of two and the norm exactly
1) and 0 in E_pad further columns.  The dot product of two rows is (E0 - 2 h) / E0 with h their Hamming distance, and every partial
sum of it is a multiple of 1 / E0 below 2: exact in fp32 in any summation order.  Metric 0 gives d = 2 (1 - s) = 4 h / E0 exactly
(h / 16 at E0 = 64), so a threshold at a multiple of 1/16 sits ON attainable distances and the strict ``d < threshold`` is decided.
Scaled by 1 + 2^-5 the dots become k / E0 (1 + 2^-4 + 2^-10): at most 18 significant bits, still exact, and |s| reaches
1.0634765625 > 1, which exercises the clamp.

Random unit rows: with the same fp32 inputs upcast to fp64, |s32 - s64| <= gamma_E sum |a_i b_i| (Higham, Accuracy and Stability of
Numerical Algorithms, 2nd ed., eq. 3.5), which turns into an interval for the fp32 distance; a (pair, threshold) whose fp32
threshold lies in that interval is *ambiguous* and is the only thing a comparison with fp64 may excuse."""
import functools
from fractions import Fraction

import numpy as np

from oracle.facenet_oracle import _fma32

ROWS = ("tp", "tn", "fp", "fn")
U32 = 2.0 ** -24
ACOS_EPS = 2.0 ** -20          # four fp32 ulps at pi: a deliberate over-estimate of acosf's error
CAP = 0.005                    # ambiguous (pair, threshold) incidences per pair of a random case


# ---- lattice rows ------------------------------------------------------------------------------------------------------------
def lattice_classes(sizes, seed, flips, E_pad=0, scale=1.0, E0=64):
    """-> (emb fp32 [n, E0 + E_pad] sorted by class, starts int [C + 1], H int [n, n] Hamming distances).

    Class c is a random sign centre with up to ``flips`` flipped signs per row.  Planted where the class is large enough: row 1
    duplicates row 0 (d = 0), row 2 is row 0 negated (h = E0: s = -1, d = 4), row 3 differs from row 0 in exactly E0 / 2 places
    (s = 0, d = 2)."""
    assert E0 in (4, 16, 64)
    rng = np.random.default_rng(seed)
    signs = []
    for n in sizes:
        centre = rng.integers(0, 2, E0) * 2 - 1
        rows = np.tile(centre, (n, 1))
        for r in range(n):
            k = int(rng.integers(0, flips + 1))
            rows[r, rng.choice(E0, size=min(k, E0), replace=False)] *= -1
        if n >= 2:
            rows[1] = rows[0]
        if n >= 3:
            rows[2] = -rows[0]
        if n >= 4:
            rows[3] = rows[0]
            rows[3, :E0 // 2] *= -1
        signs.append(rows)
    S = np.concatenate(signs).astype(np.int64)
    amp = np.float32(scale) * np.float32(E0 ** -0.5)
    assert float(amp) == float(np.float32(scale)) * E0 ** -0.5          # a power of two times the scale: no rounding
    emb = np.zeros((len(S), E0 + E_pad), np.float32)
    emb[:, :E0] = S.astype(np.float32) * amp
    starts = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return emb, starts, (E0 - S @ S.T) // 2


@functools.lru_cache(maxsize=None)
def many_class_pool():
    """-> (sizes, emb [825, 20], starts, H): 300 classes of sizes cycling 1, 2, 3, 5; the cycle shifts by one from class 256 on, so
    that a diagonal workgroup of the class-pair walk (stride 256) meets a one-row class and then a populated one, or the reverse.
    1 050 genuine and 338 850 impostor pairs; 44 850 off-diagonal class pairs over 2048 workgroups, 300 diagonal ones over 256.
    Shared by its callers: not to be written to."""
    sizes = [(1, 2, 3, 5)[(c + (c >= 256)) % 4] for c in range(300)]
    return (sizes,) + lattice_classes(sizes, seed=12, flips=8, E_pad=4, E0=16)


def exact_dots(H, E0=64, scale=1.0):
    """The unclamped dot products of the lattice rows, exact in fp64 (and in fp32)."""
    p = Fraction(float(np.float32(scale))) ** 2
    assert p.denominator & (p.denominator - 1) == 0 and p.numerator < 2 ** 12
    return (E0 - 2 * H) * float(p) / E0                                   # an integer of <= 7 bits times <= 12 bits, over 2^k


def _class_of(starts):
    return np.repeat(np.arange(len(starts) - 1), np.diff(starts))


def _pairs(starts, full=False):
    """Row pairs (a, b) the kernels evaluate and their class-pair slot i (i + 1) / 2 + k, i >= k: the strict upper triangle of a
    diagonal class pair and the whole rectangle otherwise; ``full``: the whole square of a diagonal pair too (fn_f2f_pair_counts)."""
    cls = _class_of(starts)
    n = len(cls)
    ca, cb = cls[:, None], cls[None, :]
    keep = (ca >= cb) if full else ((ca > cb) | ((ca == cb) & (np.arange(n)[None, :] > np.arange(n)[:, None])))
    a, b = np.nonzero(keep)
    return a, b, cls[a] * (cls[a] + 1) // 2 + cls[b]


def _bins(H, a, b, thr32, metric, E0, scale):
    """First n with thr[n] > d for every listed pair: integer arithmetic for metric 0, fp64 arccos of the exact s for metric 1."""
    thr = np.asarray(thr32, np.float32).astype(np.float64)
    assert np.all(np.diff(thr) >= 0)
    p = Fraction(float(np.float32(scale))) ** 2
    den = E0 * p.denominator                                              # s = k p.num / den, a power of two below
    assert den & (den - 1) == 0
    k = (E0 - 2 * H[a, b]) * p.numerator
    if metric == 0:
        d_num = 2 * (den - np.clip(k, -den, den))                         # d = d_num / den
        return np.searchsorted(thr * den, d_num, side="right")            # thr * den is exact: den is a power of two
    return np.searchsorted(thr, np.arccos(np.clip(k / den, -1.0, 1.0)), side="right")


def exact_counts(H, starts, thr32, metric, E0=64, scale=1.0, full=False, fold=None, F=0):
    """-> (counts int [C (C + 1) / 2, T]: count(d < thr[n]) per class pair (i >= k), P int [C (C + 1) / 2]: its number of pairs).
    With ``fold`` (int [n], the fold each row is held out in): counts [F, pairs, T] over the pairs of each fold's training part
    (neither row held out in f), the ``total - touch_f`` of validation_folds_oracle.onepass counted directly."""
    C, T = len(starts) - 1, len(thr32)
    a, b, slot = _pairs(starts, full)
    bins = _bins(H, a, b, thr32, metric, E0, scale)
    npairs = C * (C + 1) // 2

    def table(sel):
        h = np.zeros((npairs, T + 1), np.int64)
        np.add.at(h, (slot[sel], bins[sel]), 1)
        return np.cumsum(h[:, :T], axis=1)
    if fold is None:
        return table(slice(None)), np.bincount(slot, minlength=npairs)
    fold = np.asarray(fold)
    return np.stack([table((fold[a] != f) & (fold[b] != f)) for f in range(F)]), None


def _slots(C):
    i, k = np.tril_indices(C)
    return i, k                                                            # slot order i (i + 1) / 2 + k


def _sum_tables(counts, P, w_diag, w_off, C):
    """tp / tn / fp / fn of one matrix: class pairs with P < 1 skipped.  Summed in extended precision and rounded once, so the
    fp64 result is within 2^-53 of the exact sum.  -> (table [4, T], terms [4]: contributing class pairs per row, max weight)."""
    i, k = _slots(C)
    diag, live = i == k, P >= 1
    out = np.zeros((4, counts.shape[1]))
    terms = np.zeros(4, np.int64)
    wmax = 0.0
    for rows, sel, w in (((0, 3), diag & live, w_diag), ((2, 1), ~diag & live, w_off)):
        if not sel.any():
            continue
        c, p = counts[sel].astype(np.float64), P[sel].astype(np.float64)[:, None]
        wt = (P[sel].astype(np.float64) * w)[:, None]
        out[rows[0]] = (c / wt).astype(np.longdouble).sum(axis=0).astype(np.float64)
        out[rows[1]] = ((p - c) / wt).astype(np.longdouble).sum(axis=0).astype(np.float64)
        terms[list(rows)] = int(sel.sum())
        wmax = max(wmax, float(wt.max()))
    return out, terms, wmax


def weighted_tables(counts, P, C):
    """[4, T] tp / tn / fp / fn in the kernel's class-balanced units (weight P C on the diagonal, P C (C - 1) / 2 off it), the
    number of class pairs behind each row and the largest weight."""
    return _sum_tables(counts, np.asarray(P), float(C), C * (C - 1) / 2.0, C)


def train_tables(starts, fold, F):
    """(train_rows int [C, F], train_classes int [F]) of a fold array over rows sorted by class."""
    C = len(starts) - 1
    held = np.zeros((C, F), np.int64)
    np.add.at(held, (_class_of(starts), np.asarray(fold)), 1)
    rows = np.diff(starts)[:, None] - held
    return rows, (rows > 0).sum(axis=0)


def fold_weights(starts, fold, F):
    """[(P int [pairs], C_f)] per fold: the pairs of every class pair and the classes left in the fold's training part."""
    C = len(starts) - 1
    rows, Cf = train_tables(starts, fold, F)
    i, k = _slots(C)
    return [(np.where(i == k, rows[i, f] * (rows[i, f] - 1) // 2, rows[i, f] * rows[k, f]), int(Cf[f])) for f in range(F)]


def weighted_tables_folds(counts, starts, fold, F):
    """The fold variant: counts [F, pairs, T] from exact_counts(fold=...), weights from the rows and classes left in each training
    part (validation_folds_oracle.onepass).  -> (tables [F, 4, T], terms [F, 4], max weight)."""
    C = len(starts) - 1
    out, terms, wmax = [], [], 0.0
    for f, (P, Cf) in enumerate(fold_weights(starts, fold, F)):
        t, n, w = _sum_tables(counts[f], P, float(Cf), Cf * (Cf - 1) / 2.0, C)
        out.append(t)
        terms.append(n)
        wmax = max(wmax, w)
    return np.stack(out), np.stack(terms), wmax


def lattice_thresholds(metric, E0=64, scale=1.0):
    """Metric 0: every multiple of 1/16 from 0 to 4 plus 4.5 (66 values; every attainable distance sits on one).  Metric 1: 0,
    the fp32 midpoints between arccos of adjacent attainable s, 3.2 (no attainable distance within reach of acosf's error)."""
    if metric == 0:
        return np.concatenate([np.arange(65) / 16.0, [4.5]]).astype(np.float32)
    s = np.clip(exact_dots(np.arange(E0 + 1), E0, scale), -1.0, 1.0)
    d = np.unique(np.arccos(s))
    return np.concatenate([[0.0], (d[:-1] + d[1:]) / 2, [3.2]]).astype(np.float32)


# ---- random unit rows: the fp32 chain and the proven allowance -----------------------------------------------------------------
def fp32_chain(A, B):
    """dot(A_i, B_j) as the kernels compute it: one fmaf chain over ascending e from 0, every step an exact IEEE fp32 fma."""
    A, B = np.asarray(A, np.float32), np.asarray(B, np.float32)
    acc = np.zeros((len(A), len(B)), np.float32)
    for e in range(A.shape[1]):
        acc = _fma32(A[:, e, None], B[None, :, e], acc)
    return acc


def gamma(E):
    return E * U32 / (1 - E * U32)


def dot_bound(emb32):
    """(s64 [n, n], delta [n, n]): fp64 dots of the fp32 rows and gamma_E sum |a_i b_i| per pair."""
    A = np.asarray(emb32, np.float32).astype(np.float64)
    return A @ A.T, gamma(A.shape[1]) * (np.abs(A) @ np.abs(A).T)


def distance_interval(s, delta, metric):
    """[lo, hi] that holds the fp32 distance of a pair whose fp32 dot lies within delta of s."""
    up, dn = np.clip(s + delta, -1.0, 1.0), np.clip(s - delta, -1.0, 1.0)
    if metric == 0:
        return 2 * (1 - up) - 4 * U32, 2 * (1 - dn) + 4 * U32
    return np.arccos(up) - ACOS_EPS, np.arccos(dn) + ACOS_EPS


def distance64(s, metric):
    s = np.clip(s, -1.0, 1.0)
    return 2 * (1 - s) if metric == 0 else np.arccos(s)


def distance32(s32, metric):
    """The kernels' fp32 distance from an fp32 dot (the host's float32 arccos stands in for acosf)."""
    sc = np.clip(np.asarray(s32, np.float32), np.float32(-1), np.float32(1))
    return (np.float32(2) * (np.float32(1) - sc)).astype(np.float32) if metric == 0 else np.arccos(sc).astype(np.float32)


def ambiguous_mask(emb32, starts, thr32, metric):
    """(a, b, slot, amb bool [pairs, T]): for every evaluated row pair, the thresholds that lie in its fp32 distance interval."""
    s, delta = dot_bound(emb32)
    a, b, slot = _pairs(starts)
    lo, hi = distance_interval(s[a, b], delta[a, b], metric)
    thr = np.asarray(thr32, np.float32).astype(np.float64)[None, :]
    return a, b, slot, (lo[:, None] <= thr) & (thr <= hi[:, None])


def ambiguity(emb32, starts, thr32, metric, fold=None, F=0):
    """int [C (C + 1) / 2, T]: ambiguous row pairs per class pair and threshold; with ``fold`` [F, ...] over each training part."""
    C = len(starts) - 1
    a, b, slot, amb = ambiguous_mask(emb32, starts, thr32, metric)

    def table(sel):
        out = np.zeros((C * (C + 1) // 2, amb.shape[1]), np.int64)
        np.add.at(out, slot[sel], amb[sel].astype(np.int64))
        return out
    if fold is None:
        return table(slice(None))
    fold = np.asarray(fold)
    return np.stack([table((fold[a] != f) & (fold[b] != f)) for f in range(F)])


def counts64(emb32, starts, thr32, metric, fold=None, F=0):
    """(counts [pairs, T], P [pairs]) from the fp64 distances of the fp32 rows against the fp32 thresholds; with ``fold``
    (counts [F, pairs, T], None) over each training part."""
    C, T = len(starts) - 1, len(thr32)
    s, _ = dot_bound(emb32)
    a, b, slot = _pairs(starts)
    bins = np.searchsorted(np.asarray(thr32, np.float32).astype(np.float64), distance64(s[a, b], metric), side="right")

    def table(sel):
        h = np.zeros((C * (C + 1) // 2, T + 1), np.int64)
        np.add.at(h, (slot[sel], bins[sel]), 1)
        return np.cumsum(h[:, :T], axis=1)
    if fold is None:
        return table(slice(None)), np.bincount(slot, minlength=C * (C + 1) // 2)
    fold = np.asarray(fold)
    return np.stack([table((fold[a] != f) & (fold[b] != f)) for f in range(F)]), None


def want_range(dots, starts, fold=None, F=0):
    """(min, max) of the unclamped dots over the pairs a kernel evaluates: all of them, or for the fold kernel with F = 2 only the
    pairs held out in the same fold (the others are in no training part).  None when there is no such pair."""
    a, b, _ = _pairs(starts)
    if fold is not None and F == 2:
        same = np.asarray(fold)[a] == np.asarray(fold)[b]
        a, b = a[same], b[same]
    return (float(dots[a, b].min()), float(dots[a, b].max())) if len(a) else None


def allowance(amb, P, C, left=None):
    """[4, T]: what the ambiguous pairs can move each table entry, sum over class pairs of amb / weight (a flipped pair moves tp and
    fn, or fp and tn, by 1 / weight each).  ``left``: the classes left in a fold's training part, which set its weights."""
    i, k = _slots(C)
    left = C if left is None else left
    diag, live = i == k, np.asarray(P) >= 1
    out = np.zeros((4, amb.shape[1]))
    for rows, sel, w in (((0, 3), diag & live, float(left)), ((2, 1), ~diag & live, left * (left - 1) / 2.0)):
        if sel.any():
            out[list(rows)] = (amb[sel] / (P[sel] * w)[:, None]).sum(axis=0)
    return out


# the random cases: (class sizes, E); seed = len(sizes), the pool recipe of tests/validation_folds_oracle.py.  The ambiguous share
# of each was measured on the CPU before it was admitted (tests/test_pair_lattice_host.py re-proves the cap on every run).
RANDOM_POOLS = [([5, 1, 9, 33, 2, 40, 7], 128), ([3] * 20, 512), ([70, 45], 96), ([150, 3, 40], 100), ([31, 32, 33, 64, 65], 67)]


def sorted_pool(sizes, E):
    """The pool of validation_folds_oracle.pool(sizes, E, seed=len(sizes)), rows sorted by class as the kernels take them."""
    from tests import validation_folds_oracle as vo
    emb, labels = vo.pool(sizes, E, seed=len(sizes))
    order = np.argsort(labels, kind="stable")
    return np.ascontiguousarray(emb[order]), np.concatenate([[0], np.cumsum(np.unique(labels, return_counts=True)[1])]).astype(np.int64), labels[order]


def random_thresholds(metric):
    return np.linspace(0, 4 if metric == 0 else np.pi, 100).astype(np.float32)
