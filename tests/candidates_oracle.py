"""NumPy restatement of fn_gallery_candidates, on identify_oracle's chain and keys.

Keys are bits(d0) << 32 | row as in identify_oracle.search; a skipped row's key is all ones.  best(q, c) is the smallest key over
the rows of label c; the answer is the k labels with the smallest best, ascending, each through the row in that key; tail row -1,
distance +inf, label -1.  Nothing here comes from the product."""
from __future__ import annotations

import numpy as np

from tests.identify_oracle import NONE, chain_similarities, distances


def label_best(q, g, labels, skip=None, s=None):
    """-> (best uint64 [Q, C]: the smallest admissible key of every label code, all ones without one; uniq [C]: the sorted
    labels; s [Q, G])."""
    s = chain_similarities(q, g) if s is None else s
    _, d0 = distances(s)
    Q, G = s.shape
    keys = (d0.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.arange(G, dtype=np.uint64)[None, :]
    if skip is not None:
        skip = np.asarray(skip)
        hit = (skip >= 0) & (skip < G)
        keys[np.nonzero(hit)[0], skip[hit]] = NONE
    uniq, codes = np.unique(np.asarray(labels), return_inverse=True)
    best = np.full((Q, len(uniq)), NONE, dtype=np.uint64)
    np.minimum.at(best, (np.arange(Q)[:, None], codes.reshape(1, -1)), keys)
    return best, uniq, s


def candidates(q, g, labels, k, metric=0, skip=None, s=None):
    """-> dict: dist [Q, k] (metric 0: d0 bit for bit, float32; metric 1: float64 arccos of the bit-exact sc), rows int32 [Q, k],
    labels int64 [Q, k], sc float32 [Q, k] (NaN in the tail), s [Q, G]."""
    best, uniq, s = label_best(q, g, labels, skip, s)
    sc, d0 = distances(s)
    Q, C = best.shape
    order = np.argsort(best, axis=1, kind="stable")[:, :k]
    top = np.take_along_axis(best, order, axis=1)
    if k > C:
        top = np.concatenate([top, np.full((Q, k - C), NONE, np.uint64)], axis=1)
        order = np.concatenate([order, np.zeros((Q, k - C), order.dtype)], axis=1)
    valid = top != NONE
    at = np.where(valid, top & np.uint64(0xFFFFFFFF), 0).astype(np.int64)
    rows = np.where(valid, at, -1).astype(np.int32)
    sel_sc = np.where(valid, np.take_along_axis(sc, at, axis=1), np.float32(np.nan)).astype(np.float32)
    sel_d0 = np.where(valid, np.take_along_axis(d0, at, axis=1), np.float32(np.inf)).astype(np.float32)
    dist = sel_d0 if metric == 0 else np.where(valid, np.arccos(sel_sc.astype(np.float64)), np.inf)
    return {"dist": dist, "rows": rows, "labels": np.where(valid, uniq[order], -1).astype(np.int64), "sc": sel_sc, "s": s}


def identity_ranks(q, qlabels, g, labels, skip=None, s=None):
    """int64 [Q]: the number of distinct impostor labels whose best key is below the best key of the query's own label, the
    0-based identity-level rank of the first mate; -1 when the query's label has no admissible row."""
    best, uniq, _ = label_best(q, g, labels, skip, s)
    ranks = np.full(best.shape[0], -1, dtype=np.int64)
    for i, label in enumerate(np.asarray(qlabels).tolist()):
        c = np.nonzero(uniq == label)[0]
        if len(c) and best[i, c[0]] != NONE:
            ranks[i] = int(sum(1 for o in range(best.shape[1]) if o != c[0] and best[i, o] < best[i, c[0]]))
    return ranks
