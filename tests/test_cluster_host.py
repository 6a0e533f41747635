"""Face clustering without a device: the NumPy oracle of fn_radius_* / fn_dbscan_* (tests/cluster_oracle.py) against
sklearn.cluster.DBSCAN and against its own definition on constructed cases, pairwise_clustering_scores against brute force, and
the argument rules of Gallery.within / Gallery.cluster and of apps/cluster.py."""
import numpy as np
import pytest

from tests import cluster_oracle as co
from tests import identify_oracle as io


def full_matrix(x):
    _, d0 = io.distances(io.chain_similarities(x, x))
    return d0


@pytest.mark.parametrize("case", co.BLOB_CASES)
def test_oracle_agrees_with_sklearn(case):
    """sklearn's comparison is <=, the library's the strict <: eps moves one fp32 step down for sklearn.  Core and noise sets are
    identical, the core rows are partitioned alike, and every border row is in a cluster that holds one of its core neighbours
    (sklearn gives a border row to whichever cluster reaches it first; the library to its nearest core neighbour's)."""
    from sklearn.cluster import DBSCAN
    eps, min_samples = case[5], case[6]
    x, _, csr = co.blob_case(*case)
    labels, core = co.dbscan(csr["offsets"], csr["cols"], csr["d0"], min_samples)
    d = full_matrix(x).astype(np.float64)
    np.fill_diagonal(d, 0.0)
    ref = DBSCAN(eps=float(np.nextafter(np.float32(eps), np.float32(-np.inf))), min_samples=min_samples, metric="precomputed").fit(d)
    ref_core = np.zeros(len(x), bool)
    ref_core[ref.core_sample_indices_] = True
    assert np.array_equal(core, ref_core)
    assert np.array_equal(labels < 0, ref.labels_ < 0)
    same, ref_same = labels[core][:, None] == labels[core][None, :], ref.labels_[core][:, None] == ref.labels_[core][None, :]
    assert np.array_equal(same, ref_same)
    border = np.nonzero(~core & (labels >= 0))[0]
    assert (len(border) > 0) == (min_samples > 1)
    for i in border:
        near = csr["cols"][csr["offsets"][i]:csr["offsets"][i + 1]]
        assert labels[i] in labels[near[core[near]]] and ref.labels_[i] in ref.labels_[near[core[near]]]
    # ids ascend with each cluster's smallest core row
    firsts = [np.nonzero(core & (labels == c))[0][0] for c in range(labels.max() + 1)]
    assert firsts == sorted(firsts) and labels.max() + 1 == len(set(ref.labels_[ref.labels_ >= 0]))


def bridge_rows(swap):
    """Two clusters of five rows (a hub and four copies of a row near it) and two bridge rows, +-1/8 entries (identify_oracle's
    tie_pool: every dot product exact).  Row 0 is at d0 = 1 of BOTH hubs, bit for bit; row 11 at 0.9375 of hub `a` and 1.0625
    of hub `b`.  At eps = 1.25 and min_samples = 5 the hubs and copies are core, the bridges are not (three neighbours: both
    hubs and each other).  swap exchanges the places of the two clusters."""
    a = io.tie_pool(1, 17)[0]
    flip = lambda v, lo, hi: np.concatenate([v[:lo], -v[lo:hi], v[hi:]])
    b = flip(a, 32, 64)
    a2, b2 = flip(a, 0, 8), flip(b, 8, 16)
    x = flip(a, 48, 64)                       # agrees with a on 0..47, with b on 0..31 and 48..63
    x2 = flip(a, 49, 64)                      # one more entry on a's side
    first, second = ([a, a2], [b, b2]) if swap else ([b, b2], [a, a2])
    rows = [x, first[0]] + [first[1]] * 4 + [second[0]] + [second[1]] * 4 + [x2]
    return np.stack(rows).astype(np.float32), (6 if not swap else 1)      # the row of hub a


@pytest.mark.parametrize("swap", [False, True])
def test_bridge_goes_to_the_nearer_cluster_and_a_tie_to_the_lower_row(swap):
    x, hub_a = bridge_rows(swap)
    d = full_matrix(x)
    assert d[0, 1] == d[0, 6] == np.float32(1.0) and d[11, hub_a] == np.float32(0.9375) and d[11, 7 - hub_a] == np.float32(1.0625)
    csr = co.self_join(x, 1.25)
    labels, core = co.dbscan(csr["offsets"], csr["cols"], csr["d0"], 5)
    assert core.tolist() == [False] + [True] * 10 + [False]
    assert labels[1:6].tolist() == [0] * 5 and labels[6:11].tolist() == [1] * 5
    assert labels[0] == 0                                        # the tie: hub row 1 before hub row 6, whichever cluster that is
    assert labels[11] == labels[hub_a]                           # the nearer hub, in the first cluster or the second
    # without the bridges' own rule nothing else changes: at min_samples = 3 the bridges are core and join everything
    one, all_core = co.dbscan(csr["offsets"], csr["cols"], csr["d0"], 3)
    assert all_core.all() and (one == 0).all()


def test_oracle_edge_cases():
    x = io.unit_rows(20, 8, 3)
    csr = co.self_join(x, 5.0)
    assert csr["offsets"][-1] == 20 * 19 and (co.dbscan(csr["offsets"], csr["cols"], csr["d0"], 1)[0] == 0).all()
    labels, core = co.dbscan(csr["offsets"], csr["cols"], csr["d0"], 21)
    assert (labels == -1).all() and not core.any()
    none = co.self_join(x, 0.0)
    labels, core = co.dbscan(none["offsets"], none["cols"], none["d0"], 1)
    assert none["offsets"][-1] == 0 and labels.tolist() == list(range(20)) and core.all()       # isolated rows: singletons
    chain = co.chain()
    c = co.self_join(chain, 2e-5)
    degree = np.diff(c["offsets"])
    assert degree.min() == 1 and degree.max() == 2
    labels, core = co.dbscan(c["offsets"], c["cols"], c["d0"], 3)
    assert core.sum() == 1022 and (labels == 0).all()
    assert (co.dbscan(c["offsets"], c["cols"], c["d0"], 1)[0] == 0).all()


def test_radius_oracle_is_the_search_oracle_cut_at_eps():
    q, g = io.unit_rows(9, 16, 1), io.unit_rows(40, 16, 2)
    ref = io.search(q, g, 40)
    eps = np.float32(ref["dist"][2, 11])                        # an attained distance: strict <
    csr = co.radius(q, g, eps, s=ref["s"])
    for i in range(9):
        want = np.sort(ref["rows"][i][ref["dist"][i] < eps])
        assert np.array_equal(csr["cols"][csr["offsets"][i]:csr["offsets"][i + 1]], want)
    up = co.radius(q, g, np.nextafter(eps, np.float32(np.inf)), s=ref["s"])
    assert up["offsets"][-1] > csr["offsets"][-1]


def brute_scores(truth, labels):
    labels = np.where(labels < 0, labels.max() + 1 + np.arange(len(labels)), labels)
    both = same_cluster = same_class = 0
    for i in range(len(labels)):
        for j in range(i + 1, len(labels)):
            c, t = labels[i] == labels[j], truth[i] == truth[j]
            both, same_cluster, same_class = both + (c and t), same_cluster + c, same_class + t
    p = both / same_cluster if same_cluster else 1.0
    r = both / same_class if same_class else 1.0
    return p, r, (2 * p * r / (p + r) if p + r else 0.0)


def test_pairwise_clustering_scores():
    from facenet_amd.statistics import pairwise_clustering_scores
    rng = np.random.default_rng(0)
    for n, nt, nc in ((60, 5, 7), (33, 33, 3), (40, 1, 6), (2, 2, 2)):
        truth = rng.integers(0, nt, n) * 3 + 100                # class names need not be 0 .. C - 1
        labels = rng.integers(-1, nc, n)
        assert pairwise_clustering_scores(truth, labels) == brute_scores(truth, labels)
    assert pairwise_clustering_scores([0, 0, 1, 1], [0, 0, 1, 1]) == (1.0, 1.0, 1.0)
    assert pairwise_clustering_scores(["a", "a", "b", "b"], [-1, -1, -1, -1]) == (1.0, 0.0, 0.0)      # noise rows are singletons
    assert pairwise_clustering_scores([0, 0, 1, 1], [0, 0, 0, 0]) == (2 / 6, 1.0, 0.5)
    big = np.arange(200000) // 2                                 # exact integers where float32 counting would not be
    assert pairwise_clustering_scores(big, big) == (1.0, 1.0, 1.0)
    with pytest.raises(ValueError, match="equal length"):
        pairwise_clustering_scores([0, 1], [0])
    with pytest.raises(ValueError, match="integers"):
        pairwise_clustering_scores([0, 1], [0.5, 1.0])


def test_gallery_argument_rules():
    from facenet_amd import _lib
    from facenet_amd.recognize import Clustering, Gallery, check_edges
    emb = io.unit_rows(6, 8, 1)
    gal = Gallery(emb, device="cpu")
    with pytest.raises(ValueError, match="2-D"):
        gal.within(emb[0], 1.0)
    with pytest.raises(ValueError, match="embedding lengths differ"):
        gal.within(io.unit_rows(2, 12, 1), 1.0)
    with pytest.raises(ValueError, match="skip must be 6 integers"):
        gal.within(emb, 1.0, skip=[0, 1])
    with pytest.raises(ValueError, match="NaN"):
        gal.within(emb, float("nan"))
    with pytest.raises(ValueError, match="max_edges"):
        gal.within(emb, 1.0, max_edges=-1)
    with pytest.raises(_lib.FacenetHipError, match="no CPU fallback"):
        gal.within(emb, 1.0)
    offsets, rows, dist = gal.within(np.zeros((0, 8), np.float32), 1.0)
    assert offsets.tolist() == [0] and rows.shape == (0,) and rows.dtype == np.int32 and dist.dtype == np.float32
    with pytest.raises(ValueError, match="needs a threshold or a classifier"):
        gal.cluster()
    with pytest.raises(ValueError, match="not both"):
        gal.cluster(threshold=1.0, classifier=object())
    for bad in (0, -3, 1.5, True, None):
        with pytest.raises(ValueError, match="min_samples"):
            gal.cluster(threshold=1.0, min_samples=bad)
    with pytest.raises(ValueError, match="FaceToFaceNormalizedEmbeddingsClassifier"):
        gal.cluster(classifier=object())
    # max_edges: the message names nnz and says what to do; 2^31 always raises
    check_edges(10, None), check_edges(10, 10), check_edges(2 ** 31 - 1)
    with pytest.raises(ValueError, match=r"nnz = 11 .* max_edges = 10: choose a smaller eps"):
        check_edges(11, 10)
    with pytest.raises(ValueError, match=r"nnz = 2147483648 .* choose a smaller eps"):
        check_edges(2 ** 31, None)
    with pytest.raises(ValueError, match=r"nnz = 2147483648"):
        check_edges(2 ** 31, 2 ** 40)
    c = Clustering(np.array([0, -1, 1, 0, 1, 1]), np.array([1, 0, 1, 0, 1, 1], bool), 2, 1, 3, 1.0, 2, None, None, None)
    assert c.sizes.tolist() == [2, 3] and c.members(1).tolist() == [2, 4, 5] and c.members(-1).tolist() == [1]
    with pytest.raises(ValueError, match="cluster 2"):
        c.members(2)
    assert "Number of clusters 2" in repr(c)


def test_app_options(tmp_path):
    from facenet_amd.apps import cluster as app
    base = {"embeddings": {"path": "~/e/emb.npz"}, "cluster": {"threshold": 1.1}}
    c = app.load_options(overrides=base)
    assert c.cluster.min_samples == 1 and c.cluster.metric == 0 and c.cluster.classifier is None
    assert c.file == c.embeddings.path.parent / "clusters.npz" and "~" not in str(c.file)
    c = app.load_options(overrides={"dataset": {"path": "photos"}, "model": {"path": "m/best.npz"},
                                    "cluster": {"classifier": "~/c.npz", "min_samples": 3, "metric": 0}})
    assert str(c.file) == "photos_best/clusters.npz" and c.cluster.threshold is None and "~" not in str(c.cluster.classifier)
    with pytest.raises(ValueError, match="embeddings.path .* or dataset.path"):
        app.load_options(overrides={"cluster": {"threshold": 1.0}})
    with pytest.raises(ValueError, match="embeddings.path .* or dataset.path"):
        app.load_options(overrides=dict(base, dataset={"path": "photos"}))
    with pytest.raises(ValueError, match="cluster.threshold or cluster.classifier"):
        app.load_options(overrides={"embeddings": {"path": "e.npz"}})
    with pytest.raises(ValueError, match="cluster.threshold or cluster.classifier"):
        app.load_options(overrides=dict(base, cluster={"threshold": 1.0, "classifier": "c.npz"}))
    for bad in (0, 2.5, True):
        with pytest.raises(ValueError, match="min_samples"):
            app.load_options(overrides=dict(base, cluster={"threshold": 1.0, "min_samples": bad}))
    with pytest.raises(ValueError, match="Undefined similarity metric 2"):
        app.load_options(overrides=dict(base, cluster={"threshold": 1.0, "metric": 2}))
    with pytest.raises(ValueError, match="must be an .npz"):
        app.load_options(overrides=dict(base, file="out.h5"))
    import yaml
    cfg = tmp_path / "x.yaml"
    cfg.write_text(yaml.safe_dump({"embeddings": {"path": "e.npz"}, "cluster": {"threshold": 0.9, "min_samples": 2}, "file": "o.npz"}))
    c = app.load_options(cfg)
    assert c.cluster.threshold == 0.9 and c.cluster.min_samples == 2 and str(c.file) == "o.npz"
