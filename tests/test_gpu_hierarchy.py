"""fn_mst_* / Gallery.spanning_tree / Gallery.hdbscan on the MI355X against the NumPy oracle (tests/mst_oracle.py): the tree's edges
(sorted), weights and core distances bit for bit.  Every buffer is over-allocated and pre-filled, so a write past its end is seen."""
import ctypes as C

import numpy as np
import pytest
import torch

from facenet_amd import _lib
from facenet_amd.hierarchy import SpanningTree, edge_order
from tests import cluster_oracle as co
from tests import mst_oracle as mo
from tests.test_gpu_identify_app import detector, photos, pipeline  # noqa: F401  (the fixtures of the identification app's test)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 7
FILL_F, FILL_I, FILL_L = -77.0, -77, 0x5A5A5A5A5A5A


def _dev(a, dtype):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def log2_ceil(n):
    return int(n - 1).bit_length()


def gpu_mst(x, core=None, slab_rows=0, again=True):
    """fn_mst_init, ceil(log2 N) rounds in one call, one look at info -> (edges sorted by (bits(w), lo, hi), weights, info[:4]).
    The guard words, the invariants of every case and (``again``) that further rounds after `done` change no buffer are checked
    here."""
    lib = _lib.load()
    N, E = x.shape
    nbytes = C.c_longlong(-1)
    assert lib.fn_mst_workspace(N, slab_rows, C.byref(nbytes)) == 0 and nbytes.value >= N * 40
    words = (nbytes.value + 7) // 8
    ws = torch.full((words + GUARD,), FILL_L, dtype=torch.int64, device=DEV)
    comp = torch.full((N + GUARD,), FILL_I, dtype=torch.int32, device=DEV)
    edges = torch.full((2 * (N - 1) + GUARD,), FILL_I, dtype=torch.int32, device=DEV)
    weights = torch.full((N - 1 + GUARD,), FILL_F, dtype=torch.float32, device=DEV)
    info = torch.full((8 + GUARD,), FILL_I, dtype=torch.int32, device=DEV)
    xd, cd = _dev(x, np.float32), _dev(core, np.float32)
    assert lib.fn_mst_init(N, _ptr(comp), _ptr(info), _stream()) == 0, lib.fn_last_error()
    if N == 1:
        assert info.cpu().tolist()[:4] == [1, 0, 1, 0]
    else:
        assert info.cpu().tolist()[:4] == [0, 0, N, 0] and comp.cpu().tolist()[:N] == list(range(N))
    rounds = (_ptr(xd), N, E, _ptr(cd), slab_rows, _ptr(ws), _ptr(comp), _ptr(edges), _ptr(weights), _ptr(info))
    assert lib.fn_mst_rounds(*rounds, max(1, log2_ceil(N)), _stream()) == 0, lib.fn_last_error()
    torch.cuda.synchronize()
    done, ran, components, written = info.cpu().tolist()[:4]
    assert (done, components, written) == (1, 1, N - 1) and ran <= log2_ceil(N), (done, ran, components, written)      # Boruvka's bound
    assert (comp[:N] == 0).all()                                  # one component, named by its smallest row
    if again:
        before = [t.clone() for t in (ws, comp, edges, weights, info)]
        assert lib.fn_mst_rounds(*rounds, 3, _stream()) == 0, lib.fn_last_error()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(before, (ws, comp, edges, weights, info)))
    assert (ws[words:] == FILL_L).all() and (comp[N:] == FILL_I).all() and (edges[2 * (N - 1):] == FILL_I).all()
    assert (weights[N - 1:] == FILL_F).all() and (info[8:] == FILL_I).all()
    e, w = edges.cpu().numpy()[:2 * (N - 1)].reshape(-1, 2), weights.cpu().numpy()[:N - 1]
    # exactly N - 1 distinct edges with lo < hi that form one component
    assert (e[:, 0] < e[:, 1]).all() and (e >= 0).all() and (e < N).all() and len(set(map(tuple, e.tolist()))) == N - 1
    uf = mo.UnionFind(N)
    assert all(uf.union(a, b) for a, b in e.tolist())
    order = edge_order(e, w)
    return e[order], w[order], [done, ran, components, written]


def check_tree(x, min_samples=1, **kw):
    w, core, _ = mo.weight_matrix(x, min_samples)
    want_edges, want_weights = mo.kruskal(w)
    edges, weights, info = gpu_mst(x, core if min_samples > 1 else None, **kw)
    assert np.array_equal(edges, want_edges)
    assert np.array_equal(weights.view(np.uint32), want_weights.view(np.uint32))              # bit for bit
    return edges, weights, info


@pytest.mark.parametrize("E", [4, 36, 128, 512])
@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 130, 300])
def test_tree_shapes(N, E):
    """Ragged row and column tiles, ragged E chunks, more than one row tile; min_samples 1, 2 and 5 where N allows."""
    x = mo.rows("unit", N, E)
    for min_samples in (1, 2, 5):
        if min_samples <= N:
            check_tree(x, min_samples, again=min_samples == 2)


@pytest.mark.parametrize("min_samples", [1, 2, 5])
@pytest.mark.parametrize("N", [130, 300])
def test_tree_does_not_depend_on_the_slabs(N, min_samples):
    """slab_rows = 64: three and five slabs against one."""
    x = mo.rows("unit", N, 36)
    nbytes, one = C.c_longlong(), C.c_longlong()
    assert _lib.load().fn_mst_workspace(N, 64, C.byref(nbytes)) == 0 and _lib.load().fn_mst_workspace(N, 0, C.byref(one)) == 0
    assert nbytes.value > one.value
    many, single = check_tree(x, min_samples, slab_rows=64), check_tree(x, min_samples, again=False)
    assert np.array_equal(many[0], single[0]) and np.array_equal(many[1].view(np.uint32), single[1].view(np.uint32))


@pytest.mark.parametrize("min_samples", [1, 2, 5])
@pytest.mark.parametrize("kind,N,E", [("ties", 200, 64), ("lattice", 130, 68), ("duplicates", 130, 36), ("identical", 70, 8)])
def test_special_inputs(kind, N, E, min_samples):
    """Masses of equal weights (an inconsistent tie-break makes Boruvka close a cycle or drop an edge), |s| > 1 (the clamp),
    duplicated rows (w = 0) and all rows identical (every weight 0: the order is (lo, hi) alone)."""
    x = mo.rows(kind, N, E)
    for slab_rows in (0, 64):
        edges, weights, _ = check_tree(x, min_samples, slab_rows=slab_rows, again=False)
    if kind == "ties":
        assert len(np.unique(weights)) < N // 4
    if kind == "duplicates":                                     # a row has three copies: its fourth other row is no copy
        assert (weights == 0).any() == (min_samples < 5)
    if kind == "identical":
        assert (weights == 0).all() and np.array_equal(edges[:, 0], np.zeros(N - 1)) and np.array_equal(edges[:, 1], np.arange(1, N))
    if kind == "lattice":
        from tests.identify_oracle import chain_similarities
        assert np.abs(chain_similarities(x, x)).max() > 1


@pytest.mark.parametrize("min_samples", [1, 3])
def test_tree_of_the_chain(min_samples):
    """cluster_oracle.chain(): 1024 rows whose neighbour graph has diameter 1023.  Boruvka's bound of 10 rounds holds (gpu_mst)."""
    edges, weights, info = check_tree(co.chain(), min_samples)
    print("rounds", info[1])
    assert 0 < info[1] <= 10


def test_argument_rules():
    lib = _lib.load()
    nbytes = C.c_longlong()
    for bad in ((0, 0), (3, -1)):
        assert lib.fn_mst_workspace(*bad, C.byref(nbytes)) == -1 and lib.fn_last_error().decode() != ""
    x = torch.zeros(64, dtype=torch.float32, device=DEV)
    ws = torch.zeros(256, dtype=torch.int64, device=DEV)
    out = torch.full((16,), FILL_I, dtype=torch.int32, device=DEV)
    wts = torch.full((8,), FILL_F, dtype=torch.float32, device=DEV)
    assert lib.fn_mst_init(0, out.data_ptr(), out.data_ptr(), _stream()) == -1 and "at least 1" in lib.fn_last_error().decode()
    assert lib.fn_mst_init(3, None, out.data_ptr(), _stream()) == -1

    def rounds(N=3, E=8, off=0, slab_rows=0, work=ws.data_ptr(), edges=out.data_ptr(), n=1):
        rc = lib.fn_mst_rounds(x.data_ptr() + off, N, E, None, slab_rows, work, out.data_ptr(), edges, wts.data_ptr(), out.data_ptr(), n, _stream())
        torch.cuda.synchronize()
        return rc, lib.fn_last_error().decode()

    for kw, text in ((dict(N=0), "at least 1"), (dict(E=6), "multiple of 4"), (dict(E=516), "multiple of 4"), (dict(off=4), "16-byte aligned"),
                     (dict(slab_rows=-1), "bad arguments"), (dict(work=None), "bad arguments"), (dict(edges=None), "bad arguments"),
                     (dict(n=0), "rounds"), (dict(n=65), "rounds")):
        rc, msg = rounds(**kw)
        assert rc == -1 and text in msg, (kw, msg)
    assert (out == FILL_I).all() and (wts == FILL_F).all()        # refused without a launch


# ---- Gallery -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_samples", [1, 2, 5])
def test_gallery_spanning_tree_and_cut(min_samples):
    """N = 300: core (from the device's own top-k search), edges and weights bit for bit; cut against Gallery.cluster on the device."""
    from facenet_amd.recognize import Gallery
    x = mo.blob_rows(300, 36, seed=8)
    w, core, _ = mo.weight_matrix(x, min_samples)
    want_edges, want_weights = mo.kruskal(w)
    gal = Gallery(x, device=DEV)
    tree = gal.spanning_tree(min_samples)
    assert isinstance(tree, SpanningTree) and tree.min_samples == min_samples and 1 <= tree.rounds <= 9
    assert tree.core.dtype == np.float32 and np.array_equal(tree.core.view(np.uint32), core.view(np.uint32))
    assert tree.edges.dtype == np.int32 and np.array_equal(tree.edges, want_edges)
    assert np.array_equal(tree.weights.view(np.uint32), want_weights.view(np.uint32))
    again = gal.spanning_tree(min_samples, slab_rows=64)
    assert np.array_equal(again.edges, tree.edges) and np.array_equal(again.weights, tree.weights)
    mid = want_weights[len(want_weights) // 2]
    for t in (mid, np.nextafter(mid, np.float32(np.inf)), want_weights[len(want_weights) // 4]):
        c = gal.cluster(threshold=float(t), min_samples=min_samples)
        got = tree.cut(t)
        assert np.array_equal(c.core, tree.core < t) or min_samples == 1
        if min_samples == 1:
            assert np.array_equal(got, c.labels)
        a, b = got[c.core], c.labels[c.core]
        pairs = set(zip(a.tolist(), b.tolist()))
        assert len(pairs) == len(set(p[0] for p in pairs)) == len(set(p[1] for p in pairs)) and (b >= 0).all()
        assert (np.bincount(got)[got[~c.core]] == 1).all()
    with pytest.raises(ValueError, match="metric 0"):
        Gallery(x, metric=1, device=DEV).spanning_tree()
    one = Gallery(x[:1], device=DEV).spanning_tree()
    assert one.edges.shape == (0, 2) and one.rounds == 0 and one.cut(1.0).tolist() == [0]


def test_gallery_hdbscan():
    """End to end against the host test's expectation: the oracle's tree through SpanningTree.hdbscan, which
    tests/test_hierarchy_host.py holds to scikit-learn's tree code."""
    from facenet_amd.recognize import Gallery
    from tests.test_hierarchy_host import HDBSCAN_CASES, blob_tree
    blob, min_cluster_size, min_samples = HDBSCAN_CASES[0]
    x, _, _, tree = blob_tree(blob, min_samples, 1)
    want = tree.hdbscan(min_cluster_size)
    gal = Gallery(x, device=DEV)
    got = gal.hdbscan(min_cluster_size)                          # min_samples = None: min_cluster_size
    assert want.nrof_clusters >= 2 and got.nrof_clusters == want.nrof_clusters and got.min_samples == min_samples
    assert np.array_equal(got.labels, want.labels) and np.array_equal(got.probabilities, want.probabilities)
    assert np.array_equal(got.persistence, want.persistence)
    leaf = gal.hdbscan(min_cluster_size, min_samples=min_samples, method="leaf", allow_single_cluster=True)
    assert np.array_equal(leaf.labels, tree.hdbscan(min_cluster_size, method="leaf", allow_single_cluster=True).labels)


def _face_tree(photos, min_samples):
    w, core, _ = mo.weight_matrix(photos.emb, min_samples)
    return SpanningTree.from_edges(*mo.kruskal(w), core, min_samples=min_samples)


def test_face_pipeline_hdbscan(pipeline, photos):  # noqa: F811
    want = _face_tree(photos, 2).hdbscan(2, allow_single_cluster=True)
    clustering, faces = pipeline.cluster(photos.frames, method="hdbscan", min_cluster_size=2, allow_single_cluster=True)
    assert [(i, n) for i, n, _ in faces] == [(i, n) for i, c in enumerate(photos.per_photo) for n in range(c)]
    assert np.array_equal(clustering.labels, want.labels) and np.array_equal(clustering.probabilities, want.probabilities)
    assert pipeline.cluster(photos.frames[2:], method="hdbscan", min_cluster_size=2) == (None, [])


def test_cluster_app_hdbscan(detector, photos, tmp_path):  # noqa: F811
    """`python -m facenet_amd.apps.cluster --config x.yaml` with cluster.method hdbscan, from an embeddings file and from photographs."""
    import yaml
    from click.testing import CliRunner

    from facenet_amd.apps import cluster as app
    want = _face_tree(photos, 2).hdbscan(2)
    n = sum(photos.per_photo)
    cfg, out = tmp_path / "x.yaml", tmp_path / "result" / "c.npz"
    cfg.write_text(yaml.safe_dump({"embeddings": {"path": str(photos.root / "gallery.npz")}, "cluster": {"method": "hdbscan", "min_cluster_size": 2},
                                   "file": str(out)}))
    result = CliRunner().invoke(app.main, ["--config", str(cfg)], catch_exceptions=False)
    assert result.exit_code == 0, result.output
    z = np.load(out)
    assert sorted(z.files) == ["files", "labels", "probabilities"] and [str(f) for f in z["files"]] == photos.files
    assert z["labels"].dtype == np.int64 and np.array_equal(z["labels"], want.labels)
    assert z["probabilities"].dtype == np.float64 and np.array_equal(z["probabilities"], want.probabilities)
    assert f"number of clusters: {want.nrof_clusters}" in result.output and f"number of noise faces: {want.nrof_noise}" in result.output

    cfg.write_text(yaml.safe_dump({"dataset": {"path": str(photos.root / "photos")}, "model": {"normalize": True, "embedding_size": 128},
                                   "image": {"size": 160, "margin": 0.25}, "mtcnn": {"weights_file": detector[1]},
                                   "cluster": {"method": "hdbscan", "min_cluster_size": 2, "min_samples": 2}, "file": str(out)}))
    result = CliRunner().invoke(app.main, ["--config", str(cfg)], catch_exceptions=False)
    assert result.exit_code == 0, result.output
    z = np.load(out)
    assert sorted(z.files) == ["boxes", "face", "files", "labels", "probabilities"] and [str(f) for f in z["files"]] == photos.files
    assert z["boxes"].shape == (n, 4) and np.array_equal(z["labels"], want.labels)
