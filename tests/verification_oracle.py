"""The verification curve by sorting: what facenet_amd.statistics.VerificationCurve must return, computed
from the list of keys of each population.  A key is the bit pattern of a pair's fp32 distance; a pair is accepted at threshold t
when d < t, i.e. key(d) < key(t).  Metric-0 keys of random rows come from pair_lattice.fp32_chain + distance32 (bit-exact
restatements of the kernels' chain), lattice keys from pair_lattice.exact_dots."""
from fractions import Fraction

import numpy as np

from tests import pair_lattice as pl

BINS = 1024


def f32_key(x):
    return int(np.array([x], np.float32).view(np.uint32)[0])


def key_f32(k):
    return float(np.array([k], np.uint32).view(np.float32)[0])


def keys_of(d32):
    """fp32 distances (any shape) -> int64 keys."""
    d32 = np.ascontiguousarray(d32, dtype=np.float32)
    assert not np.signbit(d32).any()
    return d32.view(np.uint32).astype(np.int64)


def split(key_matrix, starts):
    """[n, n] keys of rows sorted by class -> (genuine, impostor): the sorted keys of the unordered pairs of distinct rows."""
    a, b, _ = pl._pairs(starts)
    cls = pl._class_of(starts)
    same = cls[a] == cls[b]
    return np.sort(key_matrix[a, b][same]), np.sort(key_matrix[a, b][~same])


def chain_keys(emb, starts):
    """Metric 0 from the host's restatement of the fp32 chain."""
    return split(keys_of(pl.distance32(pl.fp32_chain(emb, emb), 0)), starts)


def lattice_keys(H, starts, E0=64, scale=1.0, metric=0):
    dots = pl.exact_dots(H, E0, scale)
    assert np.array_equal(dots.astype(np.float32).astype(np.float64), dots)
    return split(keys_of(pl.distance32(dots.astype(np.float32), metric)), starts)


def below(keys, k):
    return int(np.searchsorted(keys, k, side="left"))


def tar_at_far(gen, imp, f):
    Gn, I = len(gen), len(imp)
    m = int(Fraction(float(f)) * I)
    if m >= I:
        t, fa, ta = float("inf"), I, Gn
    else:
        k = int(imp[m])                                   # the (m + 1)-th smallest impostor key
        t, fa, ta = key_f32(k), below(imp, k), below(gen, k)
        assert fa <= m < below(imp, k + 1)
    return {"far_target": float(f), "threshold": t, "false_accepts": fa, "true_accepts": ta, "far": fa / I, "tar": ta / Gn}


def eer(gen, imp):
    """The counts change only just above a key that occurs, and at threshold 0 nothing is accepted: t1 is one key above the first
    occurring key v with cumI(<= v) Gn >= (Gn - cumG(<= v)) I."""
    Gn, I = len(gen), len(imp)
    for v in np.unique(np.concatenate([gen, imp])):
        fa, ta = below(imp, int(v) + 1), below(gen, int(v) + 1)
        if fa * Gn >= (Gn - ta) * I:
            far, frr = fa / I, (Gn - ta) / Gn
            return {"eer": (far + frr) / 2, "eer_threshold": key_f32(int(v) + 1), "far": far, "frr": frr, "false_accepts": fa,
                    "true_accepts": ta}
    raise AssertionError("unreachable: above the largest key every pair is accepted")


def auc(gen, imp):
    """Mann-Whitney: the share of (genuine, impostor) pairs with genuine < impostor, ties counted 1/2.  A Fraction."""
    right, left = np.searchsorted(imp, gen, side="right"), np.searchsorted(imp, gen, side="left")
    twice = 2 * int((len(imp) - right).sum()) + int((right - left).sum())
    return Fraction(twice, 2 * len(gen) * len(imp))


def roc_at(gen, imp, keys):
    return [below(gen, k) for k in keys], [below(imp, k) for k in keys]


def histogram(gen, imp, lo, shift):
    """fn_pair_key_histogram's out: uint64 [R, 2, BINS + 2] = the bins, the keys below lo, the population's size."""
    out = np.zeros((len(lo), 2, BINS + 2), np.uint64)
    for r, (l, s) in enumerate(zip(lo, shift)):
        for p, keys in enumerate((gen, imp)):
            keys = np.asarray(keys, np.int64)
            b = (keys[keys >= l] - int(l)) >> int(s)
            out[r, p, :BINS] = np.bincount(b[b < BINS], minlength=BINS)
            out[r, p, BINS] = np.count_nonzero(keys < l)
            out[r, p, BINS + 1] = len(keys)
    return out
