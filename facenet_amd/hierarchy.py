"""Hierarchical clustering read from one tree: `SpanningTree` is the minimum spanning tree of a gallery's rows
under the mutual-reachability distance, built on the device by `Gallery.spanning_tree` (fn_mst_*), and everything here is host
work over its N - 1 edges: the single-linkage cut at any threshold (DBSCAN* for min_samples > 1), the SciPy linkage matrix and
HDBSCAN.  Nothing here needs a device or the library.

The edges are kept in the order (bits(w), lo, hi), which is part of the definition: the binary dendrogram merges them in that
order, and with tied weights the labels of HDBSCAN depend on it."""
from __future__ import annotations

import numpy as np

MAX_MIN_SAMPLES = 65      # core distances come from a k = min_samples - 1 <= 64 nearest search
INF = float("inf")


def edge_order(edges, weights):
    """The permutation that sorts edges (lo < hi) by (bits(w), lo, hi); weights are fp32 >= +0, so their bits order as they do."""
    bits = np.ascontiguousarray(weights, dtype=np.float32).view(np.uint32)
    return np.lexsort((edges[:, 1], edges[:, 0], bits))


class _UnionFind:
    """Union by attaching to a fresh node, as the dendrogram numbers its merges: find with path compression."""

    def __init__(self, n):
        self.parent = np.arange(2 * n - 1, dtype=np.int64) if n else np.zeros(0, np.int64)
        self.size = np.concatenate([np.ones(n, np.int64), np.zeros(max(n - 1, 0), np.int64)])
        self.next = n

    def find(self, x):
        p = self.parent
        root = x
        while p[root] != root:
            root = p[root]
        while p[x] != root:
            p[x], x = root, p[x]
        return int(root)

    def union(self, a, b):
        self.parent[a] = self.parent[b] = self.next
        self.size[self.next] = self.size[a] + self.size[b]
        self.next += 1


def _components(edges, n):
    """int [n]: a component number per row of the graph of these edges."""
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import connected_components
    graph = csr_matrix((np.ones(len(edges), np.int8), (edges[:, 0], edges[:, 1])), shape=(n, n))
    return connected_components(graph, directed=False)[1]


def first_row_ids(roots):
    """Any labelling of rows by a representative (-1: none) -> ids 0 .. C - 1 ascending with each group's smallest row."""
    roots = np.asarray(roots, dtype=np.int64)
    out = np.full(len(roots), -1, dtype=np.int64)
    keep = roots >= 0
    uniq, first, inverse = np.unique(roots[keep], return_index=True, return_inverse=True)
    rank = np.empty(len(uniq), dtype=np.int64)
    rank[np.argsort(first, kind="stable")] = np.arange(len(uniq))
    out[keep] = rank[inverse.reshape(-1)]
    return out


class HierarchicalClustering:
    """The result of `SpanningTree.hdbscan`, in the shape of `gallery.Clustering`: ``labels`` int64 [N] (cluster ids 0 ..
    nrof_clusters - 1 in ascending order of each cluster's smallest row, -1 for noise), ``probabilities`` float64 [N] (the strength
    of a row's membership: lambda of the row over the largest lambda of its cluster, 0 for noise), ``persistence`` float64
    [nrof_clusters] (each selected cluster's stability: the sum over its rows of lambda_leave - lambda_birth), ``nrof_clusters``,
    ``nrof_noise``, and the parameters."""

    def __init__(self, labels, probabilities, persistence, min_cluster_size, min_samples, method):
        self.labels, self.probabilities, self.persistence = labels, probabilities, persistence
        self.nrof_clusters = len(persistence)
        self.nrof_noise = int(np.count_nonzero(labels < 0))
        self.min_cluster_size, self.min_samples, self.method = min_cluster_size, min_samples, method

    @property
    def sizes(self):
        """int64 [nrof_clusters]: rows per cluster (noise rows are in none)."""
        return np.bincount(self.labels[self.labels >= 0], minlength=self.nrof_clusters).astype(np.int64)

    def members(self, c):
        """The rows of cluster c, ascending (c = -1: the noise rows)."""
        if not -1 <= c < self.nrof_clusters:
            raise ValueError(f"cluster {c} is not in [-1, {self.nrof_clusters})")
        return np.nonzero(self.labels == c)[0]

    def __repr__(self):
        return (f"{self.__class__.__name__}\n" + f"Number of images {len(self.labels)}\n" + f"Number of clusters {self.nrof_clusters}\n" +
                f"Number of noise images {self.nrof_noise}\n" +
                f"min_cluster_size: {self.min_cluster_size} min_samples: {self.min_samples} method: {self.method}\n")


class SpanningTree:
    """The minimum spanning tree of N rows under w(i, j) = max(d(i, j), core[i], core[j]) and the edge order (bits(w), lo, hi):
    ``edges`` int32 [N - 1, 2] with lo < hi and ``weights`` float32 [N - 1], sorted ascending by (w, lo, hi); ``core`` float32 [N]
    (the distance to the (min_samples - 1)-th nearest other row, zeros for min_samples = 1), ``rounds`` (Boruvka rounds run on
    the device) and ``min_samples``."""

    def __init__(self, edges, weights, core, rounds, min_samples):
        self.edges, self.weights, self.core = edges, weights, core
        self.rounds, self.min_samples = rounds, min_samples

    @classmethod
    def from_edges(cls, edges, weights, core=None, rounds=0, min_samples=1):
        """From the N - 1 edges of a spanning tree in any order, either end first: they are checked, oriented and sorted."""
        edges = np.asarray(edges).reshape(-1, 2)
        if edges.dtype.kind not in "iu":
            raise ValueError(f"edges must be integers, got {edges.dtype}")
        weights = np.ascontiguousarray(weights, dtype=np.float32).reshape(-1)
        n = len(edges) + 1
        if len(weights) != n - 1:
            raise ValueError(f"{n - 1} edges need {n - 1} weights, got {len(weights)}")
        core = np.zeros(n, dtype=np.float32) if core is None else np.ascontiguousarray(core, dtype=np.float32).reshape(-1)
        if len(core) != n:
            raise ValueError(f"core must hold one distance per row ({n}), got {len(core)}")
        if np.isnan(weights).any() or (weights < 0).any():
            raise ValueError("tree weights must be numbers of at least 0")
        edges = np.stack([edges.min(axis=1), edges.max(axis=1)], axis=1).astype(np.int32)
        if len(edges) and (edges[:, 0] < 0).any() or (edges[:, 1] >= n).any() or (edges[:, 0] == edges[:, 1]).any():
            raise ValueError(f"edges must join two different rows in [0, {n})")
        order = edge_order(edges, weights)
        if len(np.unique(_components(edges, n))) != 1:           # N - 1 edges in one component: a tree
            raise ValueError(f"the {n - 1} edges do not form a tree: some of them close a cycle")
        return cls(edges[order], weights[order], core, int(rounds), int(min_samples))

    @property
    def nrof_images(self):
        return len(self.core)

    def __repr__(self):
        return (f"{self.__class__.__name__}\n" + f"Number of images {self.nrof_images}\n" + f"min_samples: {self.min_samples}\n" +
                f"rounds: {self.rounds}\n")

    def cut(self, threshold):
        """Labels int64 [N] of the forest of the edges with ``w < threshold`` (strict fp32): ids 0 .. C - 1 ascend with each
        cluster's smallest row.  min_samples = 1: `Gallery.cluster(threshold, min_samples=1).labels`.  min_samples = m: DBSCAN*,
        the rows with ``core < threshold`` partitioned as `Gallery.cluster(threshold, min_samples=m)` partitions its core rows,
        every other row a singleton."""
        threshold = np.float32(threshold)
        if np.isnan(threshold):
            raise ValueError("threshold must be a number, got NaN")
        n = self.nrof_images
        keep = int(np.searchsorted(self.weights, threshold, side="left"))          # weights ascend: the edges with w < threshold
        return first_row_ids(_components(self.edges[:keep], n))

    def dendrogram(self):
        """The binary dendrogram that merges the edges in their order -> (left int64 [N - 1], right, weight float64, size): merge
        i makes node N + i of the nodes that hold the edge's lo (left) and hi (right)."""
        n = self.nrof_images
        left, right = np.empty(n - 1, np.int64), np.empty(n - 1, np.int64)
        size = np.empty(n - 1, np.int64)
        uf = _UnionFind(n)
        for i, (lo, hi) in enumerate(self.edges.tolist()):
            a, b = uf.find(lo), uf.find(hi)
            left[i], right[i], size[i] = a, b, uf.size[a] + uf.size[b]
            uf.union(a, b)
        return left, right, self.weights.astype(np.float64), size

    def linkage(self):
        """The SciPy linkage matrix float64 [N - 1, 4] of single linkage under the tree's weights, merges in the (w, lo, hi)
        order: for `scipy.cluster.hierarchy.fcluster`, `dendrogram` and the like."""
        left, right, weight, size = self.dendrogram()
        return np.stack([left.astype(np.float64), right.astype(np.float64), weight, size.astype(np.float64)], axis=1)

    def hdbscan(self, min_cluster_size=5, method="eom", allow_single_cluster=False):
        """HDBSCAN over the tree -> `HierarchicalClustering`: the condensed tree at ``min_cluster_size``, stabilities with lambda
        = 1 / w in float64 (+inf where w = 0) and the selection by excess of mass (``method='eom'``) or the leaves of the cluster
        tree (``'leaf'``), the algorithm of scikit-learn's _hdbscan/_tree.pyx on the dendrogram of `dendrogram`.
        ``allow_single_cluster``: the root may be selected, as there."""
        if isinstance(min_cluster_size, bool) or not isinstance(min_cluster_size, (int, np.integer)) or min_cluster_size < 2:
            raise ValueError(f"min_cluster_size must be an integer of at least 2, got {min_cluster_size!r}")
        if method not in ("eom", "leaf"):
            raise ValueError(f"method must be 'eom' or 'leaf', got {method!r}")
        n = self.nrof_images
        if n < 2:
            labels = np.full(n, -1, dtype=np.int64)
            return HierarchicalClustering(labels, np.zeros(n), np.zeros(0), int(min_cluster_size), self.min_samples, method)
        condensed = condense(*self.dendrogram(), int(min_cluster_size))
        with np.errstate(invalid="ignore"):
            raw, prob, stability = select_clusters(condensed, n, method, bool(allow_single_cluster))
        labels = first_row_ids(raw)
        persistence = np.zeros(int(labels.max()) + 1 if len(labels) else 0)
        for c, r in zip(labels.tolist(), raw.tolist()):
            if c >= 0:
                persistence[c] = stability[r]
        return HierarchicalClustering(labels, prob, persistence, int(min_cluster_size), self.min_samples, method)


# ---- HDBSCAN on the host: the steps of scikit-learn's sklearn/cluster/_hdbscan/_tree.pyx, in its orders of traversal, since the
# float64 sums of the stabilities and the run-length reading of a cluster's largest lambda depend on the order of the condensed rows
def _bfs(left, right, n, root):
    out, queue = [], [root]
    while queue:
        out.extend(queue)
        queue = [c for x in queue if x >= n for c in (int(left[x - n]), int(right[x - n]))]
    return out


def condense(left, right, weight, size, min_cluster_size):
    """The condensed tree: lists (parent, child, lambda, child size); clusters are numbered from N (the root) in the order they
    split off, rows keep their numbers."""
    n = len(left) + 1
    root = 2 * (n - 1)
    relabel = np.zeros(root + 1, dtype=np.int64)
    relabel[root] = n
    next_label = n + 1
    ignore = np.zeros(root + 1, dtype=bool)
    parent, child, lam, csize = [], [], [], []

    def fall_out(of, sub, value):
        for s in _bfs(left, right, n, sub):
            if s < n:
                parent.append(of), child.append(s), lam.append(value), csize.append(1)
            ignore[s] = True

    for node in _bfs(left, right, n, root):
        if node < n or ignore[node]:
            continue
        a, b, w = int(left[node - n]), int(right[node - n]), float(weight[node - n])
        value = 1.0 / w if w > 0.0 else INF
        na = int(size[a - n]) if a >= n else 1
        nb = int(size[b - n]) if b >= n else 1
        here = int(relabel[node])
        if na >= min_cluster_size and nb >= min_cluster_size:
            for c, nc in ((a, na), (b, nb)):
                relabel[c] = next_label
                parent.append(here), child.append(next_label), lam.append(value), csize.append(nc)
                next_label += 1
        elif na < min_cluster_size and nb < min_cluster_size:
            fall_out(here, a, value)
            fall_out(here, b, value)
        elif na < min_cluster_size:
            relabel[b] = here
            fall_out(here, a, value)
        else:
            relabel[a] = here
            fall_out(here, b, value)
    return (np.asarray(parent, dtype=np.int64), np.asarray(child, dtype=np.int64), np.asarray(lam, dtype=np.float64),
            np.asarray(csize, dtype=np.int64))


def select_clusters(condensed, n, method, allow_single_cluster):
    """-> (raw int64 [N]: the condensed-tree cluster of every row or -1, probabilities float64 [N], {cluster: stability})."""
    parent, child, lam, csize = condensed
    nclusters = int(parent.max()) - n + 1
    births = np.full(n + nclusters, np.nan)
    births[child] = lam
    births[n] = 0.0
    total = [0.0] * nclusters
    for p, v, s in zip(parent.tolist(), lam.tolist(), csize.tolist()):
        total[p - n] += (v - births[p]) * s
    stability = {n + i: float(t) for i, t in enumerate(total)}
    own = dict(stability)                    # excess of mass overwrites a parent's with its subtree's

    is_tree = csize > 1
    tparent, tchild = parent[is_tree], child[is_tree]
    children = {}
    for p, c in zip(tparent.tolist(), tchild.tolist()):
        children.setdefault(p, []).append(c)

    def below(node):
        out, queue = [], [node]
        while queue:
            out.extend(queue)
            queue = [c for x in queue for c in children.get(x, [])]
        return out

    nodes = sorted(stability, reverse=True)
    if not allow_single_cluster:
        nodes = nodes[:-1]
    is_cluster = {c: True for c in nodes}
    if method == "eom":
        for node in nodes:
            subtree = float(np.sum([stability[c] for c in children.get(node, [])]))
            if subtree > stability[node]:
                is_cluster[node] = False
                stability[node] = subtree
            else:
                for sub in below(node):
                    if sub != node:
                        is_cluster[sub] = False
    else:
        leaves = set(c for c in below(n) if c not in children) if len(tparent) else set()
        for c in is_cluster:                 # (no leaf at all: nothing is selected, as there)
            is_cluster[c] = c in leaves
    clusters = set(c for c, yes in is_cluster.items() if yes)

    # labels: a row belongs to the selected cluster it falls out of, or out of whose unselected descendant
    top = np.arange(n + nclusters, dtype=np.int64)           # cluster -> its selected ancestor (or the root)
    for p, c in zip(tparent.tolist(), tchild.tolist()):      # parents come before their children in the condensed order
        if c not in clusters:
            top[c] = top[p]
    raw = np.full(n, -1, dtype=np.int64)
    point = csize == 1
    for p, c, v in zip(parent[point].tolist(), child[point].tolist(), lam[point].tolist()):
        cluster = int(top[p])
        if cluster != n:
            raw[c] = cluster
        elif len(clusters) == 1 and allow_single_cluster:
            if v >= lam[parent == n].max():
                raw[c] = n

    # probabilities: lambda over the largest lambda of the LAST run of the cluster's rows in the condensed order, as there
    deaths = np.zeros(n + nclusters)
    current, largest = int(parent[0]), float(lam[0])
    for p, v in zip(parent[1:].tolist(), lam[1:].tolist()):
        if p == current:
            largest = max(largest, v)
        else:
            deaths[current] = largest
            current, largest = p, v
    deaths[current] = largest
    prob = np.zeros(n)
    for c, v in zip(child[point].tolist(), lam[point].tolist()):
        if raw[c] < 0:
            continue
        most = deaths[raw[c]]
        prob[c] = 1.0 if most == 0.0 or np.isinf(v) else min(v, most) / most
    return raw, prob, own
