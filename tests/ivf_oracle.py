"""NumPy restatement of the inverted-file index: fn_kmeans_update, the k-means loop of `ivf.kmeans` and
fn_ivf_search, on the chain similarities and keys of tests/identify_oracle.py.

fn_kmeans_update: sum[c][e] is the sequential fp64 sum, from 0.0, of (double)row[m][e] over the members m of c in ascending
row order; n2[c] the sequential fp64 sum, from 0.0 and over ascending e, of the rounded products sum[c][e] * sum[c][e];
centroid[c][e] = (float)(sum[c][e] / sqrt(n2[c])).  A list without a member, or with n2 == 0, keeps its previous centroid.

fn_ivf_search is identify_oracle.search with the keys of unprobed rows set to NONE."""
from __future__ import annotations

import numpy as np

from tests import identify_oracle as io


def kmeans_update(rows, assign, prev):
    """-> (centroids float32 [L, E], kept int32 [L]).  NumPy's float64 +, *, / and sqrt are the IEEE operations, each rounded once."""
    rows, prev = np.asarray(rows, dtype=np.float32), np.asarray(prev, dtype=np.float32)
    L, E = prev.shape
    total = np.zeros((L, E), dtype=np.float64)
    for m in range(rows.shape[0]):                       # ascending row order within every list
        total[assign[m]] = total[assign[m]] + rows[m].astype(np.float64)
    n2 = np.zeros(L, dtype=np.float64)
    for e in range(E):
        n2 = n2 + total[:, e] * total[:, e]
    kept = (np.bincount(assign, minlength=L) == 0) | (n2 == 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        new = (total / np.sqrt(n2)[:, None]).astype(np.float32)
    return np.where(kept[:, None], prev, new), kept.astype(np.int32)


def assign_rows(rows, centroids):
    """Every row's nearest centroid under (d0, centroid index): fn_gallery_search with k = 1."""
    return io.search(rows, centroids, 1)["rows"][:, 0]


def objective(rows, centroids, assign):
    """The spherical k-means objective in fp64: the sum of 1 - x . c over the rows."""
    return float((1.0 - (rows.astype(np.float64) * centroids.astype(np.float64)[assign]).sum(axis=1)).sum())


def kmeans(rows, nlist, iters=10, seed=0, history=None):
    """The loop of facenet_amd.ivf.kmeans -> (centroids, assign, info).  ``history``: a list that receives (centroids, assign)
    as they stand before each centroid update."""
    rows = np.asarray(rows, dtype=np.float32)
    G = rows.shape[0]
    centroids = rows[np.random.RandomState(seed).permutation(G)[:nlist]].copy()
    assign, moved, updates, converged = None, [], 0, False
    for _ in range(iters):
        new = assign_rows(rows, centroids)
        moved.append(G if assign is None else int((new != assign).sum()))
        assign = new
        if history is not None:
            history.append((centroids, assign))
        if moved[-1] == 0:
            converged = True
            break
        centroids, updates = kmeans_update(rows, assign, centroids)[0], updates + 1
    if not converged:
        new = assign_rows(rows, centroids)
        moved.append(G if assign is None else int((new != assign).sum()))
        assign, converged = new, moved[-1] == 0
    empty = int((np.bincount(assign, minlength=nlist) == 0).sum())
    return centroids, assign.astype(np.int32), {"iterations": updates, "moved": moved, "empty": empty, "converged": converged}


def lists_of(assign, nlist):
    """(ids int32 [G]: the original row of each stored row, list_start int32 [nlist + 1]) of an assignment."""
    assign = np.asarray(assign)
    ids = np.argsort(assign, kind="stable").astype(np.int32)
    return ids, np.concatenate([[0], np.cumsum(np.bincount(assign, minlength=nlist))]).astype(np.int32)


def ivf_search(q, g, assign, probes, k, metric=0, skip=None, s=None):
    """identify_oracle.search over the rows whose list the query probes (probes [Q, nprobe], -1: none) -> its dict; ``range``:
    (min, max) of s over the pairs evaluated, None without one."""
    s = io.chain_similarities(q, g) if s is None else s
    sc, d0 = io.distances(s)
    Q, G = s.shape
    assign, probes = np.asarray(assign), np.asarray(probes)
    probed = (assign[None, None, :] == probes[:, :, None]).any(axis=1)           # [Q, G]; -1 matches no list
    keys = (d0.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.arange(G, dtype=np.uint64)[None, :]
    keys[~probed] = io.NONE
    if skip is not None:
        skip = np.asarray(skip)
        hit = (skip >= 0) & (skip < G)
        keys[np.nonzero(hit)[0], skip[hit]] = io.NONE
    order = np.argsort(keys, axis=1, kind="stable")[:, :k]
    best = np.take_along_axis(keys, order, axis=1)
    rows = np.where(best == io.NONE, -1, order).astype(np.int32)
    if k > G:
        pad = k - G
        rows = np.concatenate([rows, np.full((Q, pad), -1, np.int32)], axis=1)
        order = np.concatenate([order, np.zeros((Q, pad), order.dtype)], axis=1)
    valid = rows >= 0
    sel_sc = np.where(valid, np.take_along_axis(sc, order, axis=1), np.float32(np.nan)).astype(np.float32)
    sel_d0 = np.where(valid, np.take_along_axis(d0, order, axis=1), np.float32(np.inf)).astype(np.float32)
    dist = sel_d0 if metric == 0 else np.where(valid, np.arccos(sel_sc.astype(np.float64)), np.inf)
    rng = (float(s[probed].min()), float(s[probed].max())) if probed.any() else None
    return {"dist": dist, "rows": rows, "sc": sel_sc, "s": s, "range": rng}


def blobs(n, E, classes, seed, spread=0.1):
    """n unit rows in `classes` tight groups (the classes cycle over the rows)."""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((classes, E))
    centres /= np.linalg.norm(centres, axis=1, keepdims=True)
    x = centres[np.arange(n) % classes] + spread * rng.standard_normal((n, E)) / np.sqrt(E)
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
