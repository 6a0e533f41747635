"""NumPy restatement of fn_radius_count / fn_radius_fill and fn_dbscan_*  and the inputs their tests share.

Radius search: s, sc and d0 are tests/identify_oracle's (the fp32 fmaf chain, every operation in fp32); (q, g) are neighbours
when d < eps with the strict fp32 <, d = d0 for metric 0.  For metric 1 d = arccos(sc) is taken in float64 and compared with
float64(eps): the device's acosf is within 4 ulp of it, so the tests place eps where no pair lies within that band.

DBSCAN, the definition the tests pin: a row is a core row when degree + 1 >= min_samples; clusters are the connected components
of the core rows under the eps-graph (scipy.sparse.csgraph.connected_components); a non-core row with a core neighbour joins the
cluster of the core neighbour with the smallest (bits(d0) << 32 | col) key; every other row is noise, label -1; cluster ids
ascend with each cluster's smallest core row."""
from __future__ import annotations

import functools

import numpy as np

from tests.identify_oracle import chain_similarities, distances

ACOS_ULPS = 8 * 2.0 ** -24          # the 4-ulp acosf rule of tests/test_gpu_loss_edges.py, as tests/test_gpu_identify.py applies it


def radius(q, g, eps, metric=0, skip=None, s=None):
    """-> dict: offsets int64 [Q + 1], cols int32 [nnz] (ascending per row), dist [nnz] (metric 0: d0 float32 bit for bit; metric
    1: float64 arccos of the bit-exact sc), d0 float32 [nnz], s [Q, G] the chain values."""
    s = chain_similarities(q, g) if s is None else s
    sc, d0 = distances(s)
    Q, G = s.shape
    if metric == 0:
        d = d0
        hit = d0 < np.float32(eps)
    else:
        d = np.arccos(sc.astype(np.float64))
        hit = d < np.float64(np.float32(eps))
    if skip is not None:
        skip = np.asarray(skip)
        ok = (skip >= 0) & (skip < G)
        hit[np.nonzero(ok)[0], skip[ok]] = False
    rows, cols = np.nonzero(hit)                                # row-major: ascending columns within each row
    offsets = np.concatenate([[0], np.cumsum(hit.sum(axis=1))]).astype(np.int64)
    return {"offsets": offsets, "cols": cols.astype(np.int32), "dist": d[rows, cols], "d0": d0[rows, cols], "s": s, "hit": hit}


def self_join(x, eps, metric=0, s=None):
    return radius(x, x, eps, metric=metric, skip=np.arange(len(x)), s=s)


def dbscan(offsets, cols, d0, min_samples):
    """-> (labels int32 [N], core bool [N]) of the self-join CSR; d0: the metric-0 distance of every CSR entry."""
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import connected_components
    offsets, cols = np.asarray(offsets, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    N = len(offsets) - 1
    degree = np.diff(offsets)
    core = degree + 1 >= min_samples
    rows = np.repeat(np.arange(N), degree)
    keep = core[rows] & core[cols]
    graph = csr_matrix((np.ones(int(keep.sum()), np.int8), (rows[keep], cols[keep])), shape=(N, N))
    _, comp = connected_components(graph, directed=False)
    root = np.full(N, -1, dtype=np.int64)                      # smallest core row of the component, for core rows
    first = {}
    for i in np.nonzero(core)[0]:
        root[i] = first.setdefault(comp[i], i)
    keys = (np.asarray(d0, dtype=np.float32).view(np.uint32).astype(np.uint64) << np.uint64(32)) | cols.astype(np.uint64)
    for i in np.nonzero(~core)[0]:
        e = np.arange(offsets[i], offsets[i + 1])
        e = e[core[cols[e]]]
        if len(e):
            root[i] = root[cols[e[np.argmin(keys[e])]]]
    ids = {r: n for n, r in enumerate(sorted(first.values()))}
    labels = np.array([ids[r] if r >= 0 else -1 for r in root], dtype=np.int32)
    return labels, core


def blobs(clusters, per, noise, E, spread, seed):
    """clusters x per unit rows around random unit centres (centre + Gaussian noise of expected length `spread`, renormalised:
    the rows' distances to their centre vary, so clusters have sparse rims) plus `noise` random unit rows, shuffled ->
    (float32 [n, E], truth int [n], -1 for the noise rows)."""
    rng = np.random.default_rng(seed)
    unit = lambda a: a / np.linalg.norm(a, axis=1, keepdims=True)
    centres = unit(rng.standard_normal((clusters, E)))
    x = unit(np.repeat(centres, per, axis=0) + spread * rng.standard_normal((clusters * per, E)) / np.sqrt(E))
    x = np.concatenate([x, unit(rng.standard_normal((noise, E)))])
    truth = np.concatenate([np.repeat(np.arange(clusters), per), np.full(noise, -1)])
    order = rng.permutation(len(x))
    return x[order].astype(np.float32), truth[order]


# clusters, rows per cluster, noise rows, E, spread, eps, min_samples
BLOB_CASES = [(7, 23, 30, 32, 0.45, 0.35, 4), (7, 23, 30, 32, 0.45, 0.35, 1), (5, 40, 17, 128, 0.6, 0.55, 6), (9, 11, 10, 8, 0.3, 0.12, 3)]


@functools.lru_cache(maxsize=None)
def blob_case(clusters, per, noise, E, spread, eps, min_samples):
    """-> (x, truth, the self-join CSR at eps (metric 0))."""
    x, truth = blobs(clusters, per, noise, E, spread, seed=100 * clusters + per)
    return x, truth, self_join(x, eps)


def chain(n=1024, seed=5):
    """n rows (cos t, sin t, 0, 0), t = i pi / n, in a seeded permutation: at eps = 2e-5 only consecutive angles are neighbours."""
    t = np.arange(n) * np.pi / n
    x = np.stack([np.cos(t), np.sin(t), np.zeros(n), np.zeros(n)], axis=1).astype(np.float32)
    return x[np.random.default_rng(seed).permutation(n)]


def metric1_eps(q, g, quantile, skip=None, s=None):
    """An fp32 eps for metric 1 in the middle of the widest gap among the sorted float64 arccos values around `quantile`, with
    the assertion that no pair lies within the acosf band of it."""
    s = chain_similarities(q, g) if s is None else s
    sc, _ = distances(s)
    d = np.sort(np.arccos(sc.astype(np.float64)).ravel())
    mid = int(quantile * (len(d) - 1))
    lo, hi = max(0, mid - 20), min(len(d) - 1, mid + 20)
    if hi == lo:
        return np.float32(d[mid] * 1.5 + 0.1)
    gaps = np.diff(d[lo:hi + 1])
    at = lo + int(np.argmax(gaps))
    eps = np.float32((d[at] + d[at + 1]) / 2)
    band = ACOS_ULPS * np.abs(d) + 2.0 ** -24 * float(eps)
    assert (np.abs(d - np.float64(eps)) > band).all(), "a pair within the acosf band of eps"
    return eps
