"""The inverted-file index without a device: the NumPy oracle (tests/ivf_oracle.py) against identify_oracle.search, the k-means
oracle's objective, the argument errors of Gallery.kmeans / Gallery.ivf / IVFGallery, save / load, the app's options and the
C ABI's new entry points."""
import ctypes as C

import numpy as np
import pytest

from tests import identify_oracle as io
from tests import ivf_oracle as vo

CASES = [(1, 1, 4, 1, 1), (5, 63, 40, 5, 4), (17, 65, 72, 64, 8), (7, 300, 64, 10, 8)]       # Q, G, E, k, lists


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("Q,G,E,k,L", CASES)
def test_all_lists_probed_is_the_exhaustive_search(Q, G, E, k, L, metric):
    q, g = io.unit_rows(Q, E, 10 + Q), io.unit_rows(G, E, 20 + G)
    assign = np.random.default_rng(G).integers(0, L, G)
    probes = np.tile(np.random.default_rng(Q).permutation(L).astype(np.int32), (Q, 1))
    skip = np.random.default_rng(k).integers(-1, G, Q)
    for sk in (None, skip):
        ref = io.search(q, g, k, metric=metric, skip=sk)
        got = vo.ivf_search(q, g, assign, probes, k, metric=metric, skip=sk, s=ref["s"])
        assert np.array_equal(got["rows"], ref["rows"])
        assert np.array_equal(got["dist"].view(np.uint64 if metric else np.uint32), ref["dist"].view(np.uint64 if metric else np.uint32))
        assert got["range"] == (float(ref["s"].min()), float(ref["s"].max()))


def test_oracle_leaves_unprobed_rows_out():
    q, g = io.unit_rows(4, 16, 1), io.unit_rows(40, 16, 2)
    assign = np.arange(40) % 4
    probes = np.array([[0, -1], [1, 3], [-1, -1], [2, 2]], dtype=np.int32)
    got = vo.ivf_search(q, g, assign, probes, 12)
    assert set(got["rows"][0][:10] % 4) == {0} and (got["rows"][0][10:] == -1).all() and np.isposinf(got["dist"][0][10:]).all()
    assert set(got["rows"][1] % 4) == {1, 3} and (got["rows"][2] == -1).all()
    for row, lists in ((0, [0]), (1, [1, 3])):
        rows = np.nonzero(np.isin(assign, lists))[0]
        want = io.search(q[row:row + 1], g[rows], 12)
        assert np.array_equal(np.where(want["rows"][0] >= 0, rows[want["rows"][0]], -1), got["rows"][row])
    ids, list_start = vo.lists_of(assign, 4)
    assert list_start.tolist() == [0, 10, 20, 30, 40] and ids[:3].tolist() == [0, 4, 8] and ids.dtype == np.int32


def test_kmeans_update_oracle_by_hand():
    rows = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0.6, 0.8, 0, 0], [-0.6, -0.8, 0, 0], [0, 0, 0, 1]], dtype=np.float32)
    prev = np.full((4, 4), 0.5, dtype=np.float32)
    got, kept = vo.kmeans_update(rows, np.array([0, 0, 2, 2, 3]), prev)
    assert kept.tolist() == [0, 1, 1, 0]                       # list 1 has no member, list 2 sums to zero exactly
    assert np.array_equal(got[0], np.array([np.sqrt(0.5), np.sqrt(0.5), 0, 0]).astype(np.float32))
    assert np.array_equal(got[1], prev[1]) and np.array_equal(got[2], prev[2]) and np.array_equal(got[3], rows[4])


def test_kmeans_oracle_objective_does_not_increase():
    """Both steps of spherical k-means minimise sum(1 - x . c): the assignment per row, the normalised sum per list.  The fp32
    chain ranks rows with an error of at most gamma_E = E u / (1 - E u) per dot product (u = 2^-24) and a centroid is rounded
    to fp32 once (relative 2 u in a dot product), so a step may raise the fp64 objective by at most G (2 gamma_E + 4 u)."""
    G, E, L = 240, 32, 6
    rows = vo.blobs(G, E, L, seed=3)
    history = []
    centroids, assign, info = vo.kmeans(rows, L, iters=6, seed=1, history=history)
    u = 2.0 ** -24
    slack = G * (2 * E * u / (1 - E * u) + 4 * u)
    values = []
    for i, (cents, asg) in enumerate(history):
        values.append(vo.objective(rows, cents, asg))          # after an assignment step
        if i + 1 < len(history):
            values.append(vo.objective(rows, history[i + 1][0], asg))        # after the update that follows it
    assert len(values) >= 3 and all(b <= a + slack for a, b in zip(values, values[1:]))
    assert values[-1] < 0.5 * values[0]                        # tight blobs: the clustering finds them
    assert info["moved"][0] == G and info["iterations"] <= 6 and info["empty"] == int((np.bincount(assign, minlength=L) == 0).sum())
    again = vo.kmeans(rows, L, iters=6, seed=1)
    assert np.array_equal(again[0].view(np.uint32), centroids.view(np.uint32)) and np.array_equal(again[1], assign)


def test_argument_errors_need_no_device(tmp_path):
    from facenet_amd import _lib
    from facenet_amd.ivf import IVFGallery
    from facenet_amd.recognize import Gallery
    emb = io.unit_rows(6, 8, 1)
    gal = Gallery(emb, labels=[0, 0, 1, 1, 2, 2], names=["ann", "bob", "cy"], device="cpu")
    for call in (gal.kmeans, gal.ivf):
        for bad in (0, 7, -1, 2.5):
            with pytest.raises(ValueError, match=r"nlist must be an integer in \[1, 6\]"):
                call(bad)
        with pytest.raises(ValueError, match="iters must be a non-negative integer"):
            call(2, iters=-1)
        with pytest.raises(_lib.FacenetHipError, match="no CPU fallback"):
            call(2)
    cents = io.unit_rows(3, 8, 2)
    assign = np.array([2, 0, 2, 0, 0, 2])
    with pytest.raises(ValueError, match=r"centroids must be a non-empty 2-D \[nlist, 8\] array"):
        IVFGallery.from_assignment(gal, io.unit_rows(3, 12, 2), assign)
    with pytest.raises(ValueError, match="assign must be 6 integers"):
        IVFGallery.from_assignment(gal, cents, assign[:5])
    with pytest.raises(ValueError, match="assign must be 6 integers"):
        IVFGallery.from_assignment(gal, cents, assign.astype(np.float32))
    with pytest.raises(ValueError, match=r"assign must name lists in \[0, 3\)"):
        IVFGallery.from_assignment(gal, cents, np.array([0, 1, 2, 3, 0, 1]))
    with pytest.raises(ValueError, match=r"assign must name lists in \[0, 3\)"):
        IVFGallery.from_assignment(gal, cents, np.array([0, 1, 2, -1, 0, 1]))

    index = IVFGallery.from_assignment(gal, cents, assign)
    assert index.nlist == 3 and index.ids.tolist() == [1, 3, 4, 0, 2, 5] and index.list_start.tolist() == [0, 3, 3, 6]
    assert np.array_equal(index.lists.numpy(), emb[index.ids]) and index.nprobe == 8
    assert (index.nrof_images, index.nrof_classes, index.length, index.metric) == (6, 3, 8, 0)
    assert np.array_equal(index.labels, gal.labels) and index.names == gal.names and "Number of lists 3" in repr(index)
    assert index.who(np.float32(0.25), 3) == (1, "bob", 0.25, 3)               # rows are the parent's rows
    with pytest.raises(ValueError, match="ids must be a permutation"):
        IVFGallery(emb, [0, 1, 2, 3, 4, 4], [0, 6], cents[:1], device="cpu")
    with pytest.raises(ValueError, match="list_start must ascend from 0 to 6"):
        IVFGallery(emb, np.arange(6), [0, 4, 3, 6], cents, device="cpu")
    with pytest.raises(ValueError, match="ids must ascend within every list"):
        IVFGallery(emb, [1, 0, 2, 3, 4, 5], [0, 3, 6], cents[:2], device="cpu")
    with pytest.raises(ValueError, match=r"centroids must be \[2, 8\]"):
        IVFGallery(emb, np.arange(6), [0, 3, 6], cents, device="cpu")

    for bad_k in (0, 65):
        with pytest.raises(ValueError, match=r"k must be in \[1, 64\]"):
            index.search(emb, k=bad_k)
    for bad in (0, -3, 1.5):
        with pytest.raises(ValueError, match="nprobe must be an integer of at least 1"):
            index.search(emb, nprobe=bad)
        with pytest.raises(ValueError, match="nprobe must be an integer of at least 1"):
            index.identify(emb, nprobe=bad)
    with pytest.raises(ValueError, match="embedding lengths differ: queries 12, gallery 8"):
        index.search(np.ones((2, 12), np.float32))
    with pytest.raises(ValueError, match="skip must be 6 integers"):
        index.search(emb, skip=[1, 2])
    with pytest.raises(ValueError, match="not both"):
        index.identify(emb, threshold=1.0, classifier=object())
    with pytest.raises(_lib.FacenetHipError, match="no CPU fallback"):
        index.search(emb)
    dist, rows = index.search(np.zeros((0, 8), np.float32), k=3)
    assert dist.shape == (0, 3) and dist.dtype == np.float32 and rows.shape == (0, 3) and rows.dtype == np.int32
    assert index.identify(np.zeros((0, 8), np.float32)) == []
    with pytest.raises(NotImplementedError, match="the Gallery it was built from"):
        index.within(emb, 0.5)


def test_save_load_round_trip(tmp_path):
    from facenet_amd.ivf import IVFGallery
    from facenet_amd.recognize import Gallery
    emb, cents = io.unit_rows(9, 12, 4), io.unit_rows(4, 12, 5)
    files = [f"/data/{cls}/{i}.png" for cls in ("ann", "bob", "cy") for i in range(3)]
    labels = np.repeat([3, 5, 2 ** 40], 3)
    gal = Gallery(emb, labels=labels, names={3: "ann", 5: "bob", 2 ** 40: "cy"}, files=files, metric=1, device="cpu")
    index = IVFGallery.from_assignment(gal, cents, np.array([3, 1, 1, 0, 3, 3, 1, 0, 1]), nprobe=2)
    with pytest.raises(ValueError, match="saved as an .npz"):
        index.save(tmp_path / "index.h5")
    back = IVFGallery.load(index.save(tmp_path / "index.npz"), device="cpu")
    assert np.array_equal(back.lists.numpy().view(np.uint32), index.lists.numpy().view(np.uint32))
    assert np.array_equal(back.centroids.embeddings.numpy().view(np.uint32), cents.view(np.uint32))
    assert np.array_equal(back.ids, index.ids) and back.ids.dtype == np.int32 and np.array_equal(back.list_start, index.list_start)
    assert np.array_equal(back.labels, labels) and back.names == index.names and np.array_equal(back.files, index.files)
    assert (back.metric, back.nprobe, back.nlist, back.centroids.metric) == (1, 2, 4, 1)
    plain = IVFGallery.from_assignment(Gallery(emb, device="cpu"), cents, np.zeros(9, dtype=np.int64))
    back = IVFGallery.load(plain.save(tmp_path / "plain.npz"), device="cpu")
    assert back.names is None and back.files is None and np.array_equal(back.labels, np.arange(9)) and back.list_start.tolist() == [0, 9, 9, 9, 9]


def test_app_options(tmp_path):
    from click.testing import CliRunner
    from facenet_amd.apps import identify as app
    base = {"dataset": {"path": str(tmp_path / "photos")}, "gallery": {"path": str(tmp_path / "g.npz")}}
    c = app.load_options(overrides=base)
    assert c.identify.nlist is None and c.identify.nprobe is None          # off by default
    c = app.load_options(overrides=dict(base, identify={"nlist": 256, "nprobe": 4, "k": 3}))
    assert (c.identify.nlist, c.identify.nprobe, c.identify.k) == (256, 4, 3)
    assert app.load_options(overrides=dict(base, identify={"nlist": 16})).identify.nprobe is None
    for key in ("nlist", "nprobe"):
        for bad in (0, -2, 1.5, True):
            with pytest.raises(ValueError, match=f"identify.{key} must be an integer of at least 1"):
                app.load_options(overrides=dict(base, identify={"nlist": 8, key: bad}))
    with pytest.raises(ValueError, match="identify.nprobe needs identify.nlist"):
        app.load_options(overrides=dict(base, identify={"nprobe": 4}))
    seen = {}
    original = app.write_identified
    app.write_identified = lambda options: seen.update(nlist=options.identify.nlist, nprobe=options.identify.nprobe, k=options.identify.k)
    try:
        cfg = tmp_path / "x.yaml"
        cfg.write_text(f"dataset: {{path: {tmp_path}/d}}\ngallery: {{path: {tmp_path}/g.npz}}\nidentify: {{k: 2, nprobe: 3, nlist: 5}}\n")
        assert CliRunner().invoke(app.main, ["--config", str(cfg)]).exit_code == 0 and seen == {"nlist": 5, "nprobe": 3, "k": 2}
        result = CliRunner().invoke(app.main, ["--config", str(cfg), "--nlist", "64", "--nprobe", "16"])
        assert result.exit_code == 0 and seen == {"nlist": 64, "nprobe": 16, "k": 2}
    finally:
        app.write_identified = original


def test_abi_exports_and_workspace_rules():
    from facenet_amd import _lib
    lib = _lib.load()
    for name in ("fn_kmeans_update", "fn_ivf_search", "fn_ivf_search_workspace"):
        assert name in _lib.EXPORTS and hasattr(lib, name)
    assert lib.fn_abi_version() == 1
    nbytes = C.c_longlong(-1)
    assert lib.fn_ivf_search_workspace(70, 8, 3, 64, 5, C.byref(nbytes)) == 0
    pairs = 70 * 3
    assert nbytes.value >= pairs * (64 * 4 + 5 * 8 + 4) and nbytes.value % 16 == 0          # a query row, a k-list and a slot per pair
    for bad in ((0, 8, 3, 64, 5), (70, 0, 3, 64, 5), (70, 8, 0, 64, 5), (70, 8, 3, 64, 0), (70, 8, 3, 64, 65), (70, 8, 3, 6, 5),
                (70, 8, 3, 516, 5), (70, 2 ** 20 + 1, 3, 64, 5), (2 ** 27, 8, 3, 64, 5)):
        assert lib.fn_ivf_search_workspace(*bad, C.byref(nbytes)) == -1 and lib.fn_last_error().decode() != ""
    assert lib.fn_ivf_search_workspace(70, 8, 3, 64, 5, None) == -1 and "bad arguments" in lib.fn_last_error().decode()
    assert lib.fn_ivf_search_workspace(70, 8, 3, 6, 5, C.byref(nbytes)) == -1 and "multiple of 4" in lib.fn_last_error().decode()
