"""Hierarchical clustering without a device: the NumPy oracle of fn_mst_* (tests/mst_oracle.py) against
SciPy's minimum spanning tree, and `SpanningTree`, fed the oracle's tree, against the DBSCAN oracle (cut), SciPy (linkage) and
scikit-learn's HDBSCAN: its tree code on the same ordered tree (always), its public ``fit`` where no two tree weights are equal
(with tied weights the labels of binary HDBSCAN depend on the order inside a tie group, and ``fit`` keeps another order)."""
import functools

import numpy as np
import pytest

from facenet_amd.hierarchy import SpanningTree
from tests import cluster_oracle as co
from tests import mst_oracle as mo

# clusters, rows per cluster, noise rows, E, spread | min_cluster_size, min_samples: N = 150, 85, 168, 150
HDBSCAN_CASES = [((5, 27, 15, 36, 0.5), 5, 5), ((4, 19, 9, 4, 0.25), 4, 2), ((6, 25, 18, 128, 0.6), 8, 8), ((5, 27, 15, 36, 0.5), 5, 1)]
SEEDS = (1, 2, 3)


@functools.lru_cache(maxsize=None)
def blob_tree(blob, min_samples, seed):
    """-> (x, w, core, the oracle's tree as a SpanningTree)."""
    x, _ = co.blobs(*blob, seed=seed)
    w, core, _ = mo.weight_matrix(x, min_samples)
    edges, weights = mo.kruskal(w)
    return x, w, core, SpanningTree.from_edges(edges, weights, core, min_samples=min_samples)


def same_partition(a, b):
    """Noise (-1) sets identical and the other rows partitioned alike."""
    a, b = np.asarray(a), np.asarray(b)
    if not np.array_equal(a < 0, b < 0):
        return False
    keep = a >= 0
    pairs = set(zip(a[keep].tolist(), b[keep].tolist()))
    return len(pairs) == len(set(p[0] for p in pairs)) == len(set(p[1] for p in pairs))


def sklearn_tree_labels(tree, min_cluster_size, method="eom", allow_single_cluster=False):
    """scikit-learn's own tree code on the same ordered tree -> (labels, probabilities)."""
    from sklearn.cluster._hdbscan._linkage import MST_edge_dtype, make_single_linkage
    from sklearn.cluster._hdbscan._tree import tree_to_labels
    mst = np.zeros(len(tree.edges), dtype=MST_edge_dtype)
    mst["current_node"], mst["next_node"], mst["distance"] = tree.edges[:, 0], tree.edges[:, 1], tree.weights.astype(np.float64)
    with np.errstate(invalid="ignore"):
        return tree_to_labels(make_single_linkage(mst), min_cluster_size, method, allow_single_cluster)


# ---- the tree ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_samples", [1, 2, 5])
@pytest.mark.parametrize("kind,n,E", [("unit", 130, 36), ("unit", 65, 4), ("ties", 90, 64), ("chain", 200, 4)])
def test_oracle_tree_weights_agree_with_scipy(kind, n, E, min_samples):
    """The weight multiset of every minimum spanning tree is the same, so this holds whatever the ties.  SciPy reads a dense 0 as
    "no edge": the matrix goes in as w + 1 (exact in float64), which moves no comparison."""
    from scipy.sparse.csgraph import minimum_spanning_tree
    x, core, edges, weights, w = mo.tree_case(kind, n, E, min_samples)
    assert len(edges) == n - 1 and (edges[:, 0] < edges[:, 1]).all()
    assert np.array_equal(weights, w[edges[:, 0], edges[:, 1]])
    dense = w.astype(np.float64) + 1.0
    np.fill_diagonal(dense, 0.0)
    ref = minimum_spanning_tree(dense).data - 1.0
    assert len(ref) == n - 1 and np.array_equal(np.sort(ref), np.sort(weights.astype(np.float64)))
    keys = [(int(b), int(lo), int(hi)) for b, (lo, hi) in zip(weights.view(np.uint32), edges)]
    assert keys == sorted(keys)                                   # Kruskal emits in the (bits(w), lo, hi) order
    if kind == "ties":
        assert len(np.unique(weights)) < (n - 1) // 4              # masses of equal weights


def test_from_edges_orients_sorts_and_checks():
    x, core, edges, weights, _ = mo.tree_case("unit", 65, 4, 2)
    perm = np.random.default_rng(0).permutation(len(edges))
    tree = SpanningTree.from_edges(edges[perm][:, ::-1], weights[perm], core, rounds=3, min_samples=2)
    assert tree.edges.dtype == np.int32 and tree.weights.dtype == np.float32
    assert np.array_equal(tree.edges, edges) and np.array_equal(tree.weights, weights) and tree.rounds == 3 and tree.min_samples == 2
    with pytest.raises(ValueError, match="close a cycle"):
        SpanningTree.from_edges(np.concatenate([edges[:-1], edges[:1]]), weights)
    with pytest.raises(ValueError, match="two different rows"):
        SpanningTree.from_edges(np.concatenate([edges[:-1], [[3, 3]]]), weights)
    with pytest.raises(ValueError, match="weights"):
        SpanningTree.from_edges(edges, weights[:-1])
    one = SpanningTree.from_edges(np.zeros((0, 2), np.int32), np.zeros(0, np.float32))
    assert one.nrof_images == 1 and one.cut(1.0).tolist() == [0] and one.linkage().shape == (0, 4)
    assert one.hdbscan(2).labels.tolist() == [-1]


# ---- cut ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_samples", [1, 2, 5])
@pytest.mark.parametrize("case", co.BLOB_CASES[:2] + co.BLOB_CASES[3:])
def test_cut_is_dbscan_star(case, min_samples):
    """min_samples = 1: Gallery.cluster's labels element for element.  min_samples = m: the rows with core < t partitioned as
    DBSCAN partitions its core rows, every other row a singleton; ids ascend with each cluster's smallest row."""
    x, _, _ = co.blob_case(*case)
    w, core, d0 = mo.weight_matrix(x, min_samples)
    edges, weights = mo.kruskal(w)
    tree = SpanningTree.from_edges(edges, weights, core, min_samples=min_samples)
    on_a_weight = weights[len(weights) // 2]
    for t in (np.float32(case[5]), on_a_weight, np.nextafter(on_a_weight, np.float32(np.inf)), np.float32(0), np.float32(5)):
        csr = co.self_join(x, t)
        want, want_core = co.dbscan(csr["offsets"], csr["cols"], csr["d0"], min_samples)
        got = tree.cut(t)
        assert got.dtype == np.int64 and np.array_equal(got, mo.cut(edges, weights, len(x), t))
        assert np.array_equal(core < t, want_core) or (min_samples == 1 and want_core.all())      # (a row counts itself: at t <= 0 too)
        if min_samples == 1:
            assert np.array_equal(got, want)
        inside = got[want_core]
        assert same_partition(inside, want[want_core])
        sizes = np.bincount(got)
        assert (sizes[got[~want_core]] == 1).all()               # every other row is a singleton
        firsts = [np.nonzero(got == c)[0][0] for c in range(got.max() + 1)]
        assert firsts == sorted(firsts)
    below, above = tree.cut(on_a_weight), tree.cut(np.nextafter(on_a_weight, np.float32(np.inf)))
    assert below.max() > above.max()                             # strict <: the edge at the threshold stays cut
    with pytest.raises(ValueError, match="NaN"):
        tree.cut(np.nan)


# ---- linkage -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,n,E,min_samples", [("unit", 130, 36, 1), ("unit", 65, 4, 5), ("ties", 90, 64, 2)])
def test_linkage_is_scipys(kind, n, E, min_samples):
    from scipy.cluster.hierarchy import fcluster, is_valid_linkage
    _, core, edges, weights, _ = mo.tree_case(kind, n, E, min_samples)
    tree = SpanningTree.from_edges(edges, weights, core, min_samples=min_samples)
    Z = tree.linkage()
    assert Z.shape == (n - 1, 4) and Z.dtype == np.float64 and is_valid_linkage(Z, throw=True)
    assert np.array_equal(Z[:, 2], weights.astype(np.float64)) and Z[-1, 3] == n
    for t in np.unique(weights)[[0, len(np.unique(weights)) // 2, -1]]:
        # fcluster joins at d <= t, the cut at w < threshold: the cut just above t
        assert same_partition(fcluster(Z, float(t), "distance"), tree.cut(np.nextafter(t, np.float32(np.inf))))


# ---- HDBSCAN -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("blob,min_cluster_size,min_samples", HDBSCAN_CASES)
def test_hdbscan_is_sklearns_tree_code(blob, min_cluster_size, min_samples, seed):
    x, _, _, tree = blob_tree(blob, min_samples, seed)
    for method, single in (("eom", False), ("leaf", False), ("eom", True), ("leaf", True)):
        labels, prob = sklearn_tree_labels(tree, min_cluster_size, method, single)
        got = tree.hdbscan(min_cluster_size, method=method, allow_single_cluster=single)
        assert same_partition(got.labels, labels), (method, single)
        assert np.abs(got.probabilities - prob).max() <= 1e-12
        assert got.nrof_clusters == labels.max() + 1 and got.nrof_noise == np.count_nonzero(labels < 0)
        assert got.labels.dtype == np.int64 and got.probabilities.dtype == np.float64 and len(got.persistence) == got.nrof_clusters
        assert np.array_equal(got.sizes, np.bincount(got.labels[got.labels >= 0], minlength=got.nrof_clusters))
        firsts = [got.members(c)[0] for c in range(got.nrof_clusters)]
        assert firsts == sorted(firsts) and np.array_equal(got.members(-1), np.nonzero(labels < 0)[0])
        assert (got.probabilities[got.labels < 0] == 0).all() and (got.persistence >= 0).all()
    assert tree.hdbscan(min_cluster_size).nrof_clusters >= 2     # the blobs are found


def test_hdbscan_a_single_cluster():
    """One tight blob: nothing without allow_single_cluster, the root with it."""
    x, _ = co.blobs(1, 60, 0, 16, 0.3, seed=4)
    w, core, _ = mo.weight_matrix(x, 5)
    tree = SpanningTree.from_edges(*mo.kruskal(w), core, min_samples=5)
    seen = set()
    for method in ("eom", "leaf"):
        for single in (False, True):
            labels, prob = sklearn_tree_labels(tree, 10, method, single)
            got = tree.hdbscan(10, method=method, allow_single_cluster=single)
            assert same_partition(got.labels, labels) and np.abs(got.probabilities - prob).max() <= 1e-12
            seen.add((single, got.nrof_clusters))
    assert (True, 1) in seen


def distinct_weight_case():
    """A case of HDBSCAN_CASES[1]'s shape whose tree weights are all distinct: any order of the edges gives the same dendrogram."""
    blob, min_cluster_size, min_samples = HDBSCAN_CASES[1]
    for seed in range(1, 40):
        x, w, core, tree = blob_tree(blob, min_samples, seed)
        if len(np.unique(tree.weights)) == len(tree.weights):
            return seed, x, w, tree, min_cluster_size, min_samples
    raise AssertionError("no seed without a tied tree edge")


def test_hdbscan_is_sklearns_fit_without_ties():
    from sklearn.cluster import HDBSCAN
    seed, x, w, tree, min_cluster_size, min_samples = distinct_weight_case()
    assert len(np.unique(tree.weights)) == len(tree.weights)
    _, _, d0 = mo.weight_matrix(x, 1)
    d = d0.astype(np.float64)
    np.fill_diagonal(d, 0.0)
    ref = HDBSCAN(min_cluster_size=min_cluster_size, min_samples=min_samples, metric="precomputed", algorithm="brute").fit(d)
    got = tree.hdbscan(min_cluster_size)
    assert same_partition(got.labels, ref.labels_) and got.nrof_clusters >= 2


def test_hdbscan_with_exact_duplicates():
    """Lattice rows hold planted duplicates: w = 0 edges, lambda = +inf.  The labels are the tree code's."""
    from tests import pair_lattice as pl
    x = pl.lattice_classes([30, 25, 35], seed=9, flips=12)[0]
    for min_samples, min_cluster_size in ((1, 5), (2, 4)):
        w, core, _ = mo.weight_matrix(x, min_samples)
        edges, weights = mo.kruskal(w)
        assert (weights == 0).any()
        tree = SpanningTree.from_edges(edges, weights, core, min_samples=min_samples)
        for method in ("eom", "leaf"):
            labels, prob = sklearn_tree_labels(tree, min_cluster_size, method)
            got = tree.hdbscan(min_cluster_size, method=method)
            assert same_partition(got.labels, labels)
            finite = np.isfinite(prob)
            assert np.array_equal(np.isfinite(got.probabilities), finite)
            assert np.abs(got.probabilities[finite] - prob[finite]).max() <= 1e-12


@pytest.mark.parametrize("min_samples,min_cluster_size", [(1, 4), (3, 4), (5, 5)])
def test_hdbscan_with_clusters_of_duplicates(min_samples, min_cluster_size):
    """Nine rows six times over, and twenty single rows: whole clusters of copies, joined by w = 0 edges (lambda = +inf: a stability
    of +inf, and inf - inf = NaN where such a cluster is born at +inf) or by edges a rounding above 0.  Labels and probabilities are
    the tree code's; its probabilities hold no NaN here."""
    x = np.concatenate([np.tile(mo.rows("unit", 9, 16, 3), (6, 1)), mo.rows("unit", 20, 16, 4)])
    x = x[np.random.default_rng(2).permutation(len(x))]
    w, core, _ = mo.weight_matrix(x, min_samples)
    edges, weights = mo.kruskal(w)
    assert np.count_nonzero(weights == 0) >= 2 * min_cluster_size
    tree = SpanningTree.from_edges(edges, weights, core, min_samples=min_samples)
    for method, single in (("eom", False), ("leaf", False), ("eom", True)):
        labels, prob = sklearn_tree_labels(tree, min_cluster_size, method, single)
        got = tree.hdbscan(min_cluster_size, method=method, allow_single_cluster=single)
        assert same_partition(got.labels, labels) and got.nrof_clusters == 9
        assert not np.isnan(prob).any() and np.abs(got.probabilities - prob).max() <= 1e-12
        assert np.isinf(got.persistence).any()


# ---- argument rules ----------------------------------------------------------------------------------------------------------
def test_argument_errors():
    from facenet_amd.recognize import FacePipeline, Gallery
    x = mo.rows("unit", 20, 8)
    gal = Gallery(x, device="cpu")
    for bad in (0, 66, 21, 2.0, True):
        with pytest.raises(ValueError, match="min_samples"):
            gal.spanning_tree(bad)
    with pytest.raises(ValueError, match="min_samples"):
        Gallery(mo.rows("unit", 100, 8), device="cpu").spanning_tree(66)
    with pytest.raises(ValueError, match="metric 0"):
        Gallery(x, metric=1, device="cpu").spanning_tree()
    with pytest.raises(ValueError, match="metric 0"):
        Gallery(x, metric=1, device="cpu").hdbscan(5)
    for bad in (1, 0, 2.5, True):
        with pytest.raises(ValueError, match="min_cluster_size"):
            gal.hdbscan(bad)
    with pytest.raises(ValueError, match="'eom' or 'leaf'"):
        gal.hdbscan(5, method="mass")
    _, core, edges, weights, _ = mo.tree_case("unit", 65, 4, 2)
    tree = SpanningTree.from_edges(edges, weights, core)
    with pytest.raises(ValueError, match="min_cluster_size"):
        tree.hdbscan(1)
    with pytest.raises(ValueError, match="'eom' or 'leaf'"):
        tree.hdbscan(5, method="dbscan")
    with pytest.raises(ValueError, match="not in"):
        tree.hdbscan(5).members(99)
    with pytest.raises(ValueError, match="'dbscan' or 'hdbscan'"):
        FacePipeline.cluster(None, [], method="single")
    from facenet_amd import _lib
    with pytest.raises(_lib.FacenetHipError, match="no CPU fallback"):
        gal.spanning_tree(2)


def test_app_options(tmp_path):
    from facenet_amd.apps import cluster as app
    base = {"embeddings": {"path": "~/e/emb.npz"}}
    c = app.load_options(overrides=dict(base, cluster={"method": "hdbscan"}))
    assert c.cluster.method == "hdbscan" and c.cluster.min_cluster_size == 5 and c.cluster.min_samples == 5
    assert c.file == c.embeddings.path.parent / "clusters.npz" and "~" not in str(c.file)
    c = app.load_options(overrides=dict(base, cluster={"method": "hdbscan", "min_cluster_size": 8, "min_samples": 3}))
    assert c.cluster.min_cluster_size == 8 and c.cluster.min_samples == 3
    assert app._cluster_arguments(c) == {"method": "hdbscan", "min_cluster_size": 8, "min_samples": 3}
    c = app.load_options(overrides=dict(base, cluster={"threshold": 1.1}))
    assert c.cluster.method == "dbscan" and c.cluster.min_samples == 1 and app._cluster_arguments(c) == {"threshold": 1.1, "min_samples": 1}
    for extra in ({"threshold": 1.0}, {"classifier": "c.npz"}, {"threshold": 1.0, "classifier": "c.npz"}):
        with pytest.raises(ValueError, match="no cluster.threshold and no cluster.classifier"):
            app.load_options(overrides=dict(base, cluster=dict(extra, method="hdbscan")))
    with pytest.raises(ValueError, match="cluster.method"):
        app.load_options(overrides=dict(base, cluster={"method": "agglomerative", "threshold": 1.0}))
    with pytest.raises(ValueError, match="cluster.metric 0"):
        app.load_options(overrides=dict(base, cluster={"method": "hdbscan", "metric": 1}))
    for bad in (1, 2.5, True):
        with pytest.raises(ValueError, match="min_cluster_size"):
            app.load_options(overrides=dict(base, cluster={"method": "hdbscan", "min_cluster_size": bad}))
    with pytest.raises(ValueError, match="min_samples"):
        app.load_options(overrides=dict(base, cluster={"method": "hdbscan", "min_samples": 0}))
    import yaml
    cfg = tmp_path / "x.yaml"
    cfg.write_text(yaml.safe_dump({"embeddings": {"path": "e.npz"}, "cluster": {"method": "hdbscan", "min_samples": 2}, "file": "o.npz"}))
    c = app.load_options(cfg)
    assert c.cluster.min_samples == 2 and c.cluster.min_cluster_size == 5 and str(c.file) == "o.npz"
