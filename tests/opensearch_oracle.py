"""NumPy restatement of fn_mate_search and of statistics.IdentificationCurve, on identify_oracle's chain.

Keys are bits(d0) << 32 | row as in identify_oracle.search.  Row g is admissible for query q when g != skip[q]; an admissible row
is a mate when gallery_labels[g] == query_labels[q] >= 0, else an impostor.  The nearest of a population is its smallest key; the
rank is the number of impostor keys below the nearest mate's key.  The curve is plain sorting and counting.  Nothing here comes
from the product."""
from __future__ import annotations

from fractions import Fraction

import numpy as np

from tests.identify_oracle import NONE, chain_similarities, distances


def keys_of(s):
    _, d0 = distances(s)
    return (d0.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.arange(s.shape[1], dtype=np.uint64)[None, :]


def mates(q, qlabels, g, glabels, metric=0, skip=None, s=None):
    """-> dict: rows int32 [Q, 2] (mate, impostor; -1: none), dist [Q, 2] (metric 0: d0 bit for bit, float32; metric 1: float64
    arccos of the bit-exact sc; +inf: none), ranks int32 [Q] (-1: no mate), sc float32 [Q, 2] (NaN: none), s [Q, G]."""
    s = chain_similarities(q, g) if s is None else s
    sc, d0 = distances(s)
    Q, G = s.shape
    qlabels, glabels = np.asarray(qlabels), np.asarray(glabels)
    keys = keys_of(s)
    admissible = np.ones((Q, G), dtype=bool)
    if skip is not None:
        skip = np.asarray(skip)
        hit = (skip >= 0) & (skip < G)
        admissible[np.nonzero(hit)[0], skip[hit]] = False
    same = (glabels[None, :] == qlabels[:, None]) & (qlabels[:, None] >= 0)
    rows = np.full((Q, 2), -1, np.int32)
    best = np.full((Q, 2), NONE, np.uint64)
    for w, population in enumerate((admissible & same, admissible & ~same)):
        k = np.where(population, keys, NONE)
        col = np.argmin(k, axis=1)                       # keys are unique: the minimum is one column
        best[:, w] = k[np.arange(Q), col]
        rows[:, w] = np.where(best[:, w] == NONE, -1, col)
    valid = rows >= 0
    at = np.maximum(rows, 0)
    sel_sc = np.where(valid, np.take_along_axis(sc, at, axis=1), np.float32(np.nan)).astype(np.float32)
    sel_d0 = np.where(valid, np.take_along_axis(d0, at, axis=1), np.float32(np.inf)).astype(np.float32)
    dist = sel_d0 if metric == 0 else np.where(valid, np.arccos(sel_sc.astype(np.float64)), np.inf)
    below = ((admissible & ~same) & (keys < best[:, :1])).sum(axis=1)
    ranks = np.where(valid[:, 0], below, -1).astype(np.int32)
    return {"rows": rows, "dist": dist, "ranks": ranks, "sc": sel_sc, "s": s}


def leave_one_out(x, labels, metric=0):
    return mates(x, labels, x, labels, metric=metric, skip=np.arange(len(x)))


# ---- the curve: sort and count -------------------------------------------------------------------------------------------------
def populations(mate_dist, impostor_dist, ranks):
    """(mated probes, probes with an impostor) as index arrays."""
    return np.nonzero(np.asarray(ranks) >= 0)[0], np.nonzero(np.isfinite(np.asarray(impostor_dist, dtype=np.float64)))[0]


def counts_at(mate_dist, impostor_dist, ranks, threshold, rank=1):
    """(false positives, hits) at a threshold, strict fp32 <."""
    mate_dist, impostor_dist = np.asarray(mate_dist, np.float32), np.asarray(impostor_dist, np.float32)
    ranks, t = np.asarray(ranks), np.float32(threshold)
    fp = sum(1 for d in impostor_dist if np.isfinite(d) and d < t)
    hits = sum(1 for d, r in zip(mate_dist, ranks) if 0 <= r < rank and d < t)
    return fp, hits


def fnir_at_fpir(mate_dist, impostor_dist, ranks, fpirs, rank=1):
    mated, nonmated = populations(mate_dist, impostor_dist, ranks)
    M, N = len(mated), len(nonmated)
    srt = sorted(np.asarray(impostor_dist, np.float32)[nonmated].tolist())
    out = []
    for f in fpirs:
        m = int(Fraction(float(f)) * N)
        t = float(srt[m]) if m < N else float("inf")
        fp, hits = counts_at(mate_dist, impostor_dist, ranks, t, rank)
        out.append({"fpir_target": float(f), "threshold": t, "false_positives": fp, "hits": hits, "fpir": fp / N, "dir": hits / M,
                    "fnir": 1 - hits / M})
    return out


def cmc(ranks, k):
    ranks = np.asarray(ranks)
    M = int((ranks >= 0).sum())
    return np.array([int(((ranks >= 0) & (ranks <= r)).sum()) / M for r in range(k)], dtype=np.float64), len(ranks) - M


def mislabelled(mate_dist, impostor_dist, impostor_rows, ranks):
    bad = [i for i in range(len(ranks)) if ranks[i] > 0]
    bad.sort(key=lambda i: (np.float32(impostor_dist[i]), i))
    return [(i, int(impostor_rows[i]), float(mate_dist[i]), float(impostor_dist[i])) for i in bad]


def ragged_labels(sizes, seed=None):
    """Class c repeated sizes[c] times, shuffled when a seed is given."""
    labels = np.repeat(np.arange(len(sizes)), sizes)
    return labels if seed is None else np.random.default_rng(seed).permutation(labels)
