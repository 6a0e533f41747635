"""NumPy restatement of fn_mst_*  and the inputs its tests share.

Weights: s and d0 are tests/identify_oracle's (the fp32 fmaf chain, every operation in fp32); core[i] is the (min_samples - 1)-th
smallest d0 of row i to any OTHER row (0 for min_samples = 1); w(i, j) = max(d0(i, j), core[i], core[j]) in fp32.  The tree is
Kruskal's on the edges sorted by (bits(w), lo, hi), lo < hi, a strict total order: THE minimum spanning tree under it.  `cut`
is union-find over the edges with w < threshold (strict fp32), ids ascending with each cluster's smallest row."""
from __future__ import annotations

import functools

import numpy as np

from tests import cluster_oracle as co
from tests.identify_oracle import chain_similarities, distances


def core_distances(d0, min_samples):
    """float32 [N]: per row the (min_samples - 1)-th smallest distance to another row; zeros for min_samples = 1."""
    n = len(d0)
    if min_samples == 1:
        return np.zeros(n, dtype=np.float32)
    other = np.where(np.eye(n, dtype=bool), np.float32(np.inf), d0)
    return np.sort(other, axis=1)[:, min_samples - 2].astype(np.float32)


def weight_matrix(x, min_samples=1):
    """-> (w float32 [N, N] (the diagonal is meaningless), core float32 [N], d0 float32 [N, N])."""
    _, d0 = distances(chain_similarities(x, x))
    assert np.array_equal(d0, d0.T)                               # the chain is symmetric bit for bit
    core = core_distances(d0, min_samples)
    return np.maximum(np.maximum(d0, core[:, None]), core[None, :]).astype(np.float32), core, d0


class UnionFind:
    def __init__(self, n):
        self.parent = list(range(n))

    def find(self, x):
        root = x
        while self.parent[root] != root:
            root = self.parent[root]
        while self.parent[x] != root:
            self.parent[x], x = root, self.parent[x]
        return root

    def union(self, a, b):
        a, b = self.find(a), self.find(b)
        if a == b:
            return False
        self.parent[max(a, b)] = min(a, b)                        # the root is the smallest row
        return True


def kruskal(w):
    """-> (edges int32 [N - 1, 2] with lo < hi, weights float32 [N - 1]) in the (bits(w), lo, hi) order."""
    n = len(w)
    lo, hi = np.triu_indices(n, 1)
    bits = w[lo, hi].view(np.uint32)
    order = np.lexsort((hi, lo, bits))
    uf = UnionFind(n)
    edges, weights = [], []
    for e in order.tolist():
        if uf.union(int(lo[e]), int(hi[e])):
            edges.append((lo[e], hi[e]))
            weights.append(w[lo[e], hi[e]])
            if len(edges) == n - 1:
                break
    return np.asarray(edges, dtype=np.int32).reshape(-1, 2), np.asarray(weights, dtype=np.float32)


def cut(edges, weights, n, threshold):
    """int64 [n]: the components of the edges with w < threshold, ids ascending with each component's smallest row."""
    uf = UnionFind(n)
    for (a, b), w in zip(edges.tolist(), weights.tolist()):
        if np.float32(w) < np.float32(threshold):
            uf.union(a, b)
    roots = np.asarray([uf.find(i) for i in range(n)])
    return np.unique(roots, return_inverse=True)[1].reshape(-1).astype(np.int64)      # roots are smallest rows: ascending


@functools.lru_cache(maxsize=None)
def tree_case(kind, n, E, min_samples, seed=0):
    """-> (x, core, edges, weights, w) of a named input; computed once and shared."""
    x = rows(kind, n, E, seed)
    w, core, _ = weight_matrix(x, min_samples)
    edges, weights = kruskal(w)
    return x, core, edges, weights, w


def rows(kind, n, E, seed=0):
    from tests import identify_oracle as io
    from tests import pair_lattice as pl
    if kind == "unit":
        return io.unit_rows(n, E, 7000 + 13 * n + E + seed)
    if kind == "ties":                                           # E = 64: masses of equal weights
        return io.tie_pool(n, 11 + seed)
    if kind == "lattice":                                        # E = 64 + 4 of padding, scaled by 1 + 2^-5, |s| > 1: the clamp
        sizes = [n // 3, n - n // 3 - n // 4, n // 4]
        return pl.lattice_classes(sizes, seed=41 + seed, flips=32, E_pad=4, scale=1.03125)[0][np.random.default_rng(seed).permutation(n)]
    if kind == "duplicates":                                     # every row four times
        base = io.unit_rows((n + 3) // 4, E, 900 + seed)
        return np.tile(base, (4, 1))[:n][np.random.default_rng(seed).permutation(n)]
    if kind == "identical":
        return np.tile(io.unit_rows(1, E, 5 + seed), (n, 1))
    if kind == "chain":
        return co.chain(n)
    raise ValueError(kind)


def blob_rows(n, E, seed):
    """About n rows in blobs of cluster_oracle.blobs: five clusters and a tenth of noise."""
    per = (n - n // 10) // 5
    return co.blobs(5, per, n - 5 * per, E, 0.5, seed)[0]
