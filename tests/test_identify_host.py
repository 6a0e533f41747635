"""1:N identification without a device: the NumPy oracle of fn_gallery_search (tests/identify_oracle.py) against brute force in
fp64, the exact-tie pool, the adversarial order, `statistics.cmc`, the Gallery's argument errors and the app's option loading."""
import numpy as np
import pytest

from tests import identify_oracle as io


def test_oracle_agrees_with_fp64_brute_force():
    """Where the fp64 distances of neighbouring candidates are further apart than twice the fp32 chain's error bound, the
    oracle's top-k IS the fp64 order.  |s - s64| <= gamma_E sum|a b| <= gamma_E (unit rows, Cauchy-Schwarz), gamma_E =
    E u / (1 - E u), u = 2^-24; 1 - sc rounds once (<= 2 u), the doubling is exact: |d0 - d64| <= 2 gamma_E + 4 u."""
    left_out = total = 0
    for (Q, G, E, k, seed) in ((8, 200, 32, 5, 1), (5, 70, 128, 10, 2), (3, 40, 512, 8, 3)):
        q, g = io.unit_rows(Q, E, seed), io.unit_rows(G, E, 100 + seed)
        got = io.search(q, g, k)
        u = 2.0 ** -24
        bound = 2 * (E * u / (1 - E * u)) + 4 * u
        d64 = 2 * (1 - np.clip(q.astype(np.float64) @ g.astype(np.float64).T, -1, 1))
        order = np.argsort(d64, axis=1, kind="stable")
        srt = np.take_along_axis(d64, order, axis=1)
        for i in range(Q):
            total += 1
            gaps = np.diff(srt[i, :min(k + 1, G)])
            if gaps.size and gaps.min() <= 2 * bound:
                left_out += 1
                continue
            assert np.array_equal(got["rows"][i], order[i, :k]), (Q, G, E, i)
            assert np.abs(got["dist"][i].astype(np.float64) - srt[i, :k]).max() <= bound
    assert total == 16 and left_out == 0          # the share of cases the gap condition leaves out: 0 / 16 for these seeds


def test_oracle_tail_skip_and_metric():
    q, g = io.unit_rows(3, 8, 5), io.unit_rows(4, 8, 6)
    r = io.search(q, g, 6, metric=1, skip=[2, -1, 0])
    assert r["rows"].shape == (3, 6) and 2 not in r["rows"][0] and 0 not in r["rows"][2]
    assert (r["rows"][0, 3:] == -1).all() and (r["rows"][1, 4:] == -1).all() and np.isinf(r["dist"][0, 3:]).all()
    assert sorted(r["rows"][1, :4].tolist()) == [0, 1, 2, 3]
    ok = r["rows"] >= 0
    assert np.array_equal(r["dist"][ok], np.arccos(r["sc"][ok].astype(np.float64))) and np.isnan(r["sc"][~ok]).all()


def test_tie_pool_is_exact():
    pool = io.tie_pool(70, 7)
    assert pool.shape == (70, io.TIE_E) and np.array_equal(np.abs(pool), np.full_like(pool, 0.125))
    assert np.array_equal((pool.astype(np.float64) ** 2).sum(axis=1), np.ones(70))          # norm exactly 1
    s = io.chain_similarities(pool[:9], pool)
    exact = pool[:9].astype(np.float64) @ pool.astype(np.float64).T                           # multiples of 1/64: exact in fp64
    assert np.array_equal(s.astype(np.float64), exact) and np.array_equal(exact * 64, np.round(exact * 64))
    partial = np.cumsum(pool[0].astype(np.float64) * pool[1].astype(np.float64))
    assert np.array_equal(partial * 64, np.round(partial * 64)) and np.abs(partial).max() <= 1
    # equal dot products exist in numbers, so the lower-row rule is exercised
    _, d0 = io.distances(s)
    assert all(len(np.unique(row)) < len(row) for row in d0)


def test_adversarial_order_gets_nearer_row_by_row():
    q, g = io.adversarial_order(1024, 32, 11)
    assert q.shape == (3, 32) and g.shape == (1024, 32)
    _, d0 = io.distances(io.chain_similarities(q, g))
    step = np.diff(d0[0].astype(np.float64))
    assert (step <= 0).all() and (step < 0).mean() > 0.99
    assert ((np.diff(d0[1:].astype(np.float64), axis=1) < 0).mean(axis=1) > 0.9).all()
    assert np.abs(np.linalg.norm(g.astype(np.float64), axis=1) - 1).max() < 1e-6


def test_cmc_hand_case():
    from facenet_amd.statistics import cmc
    labels = np.array([0, 0, 1, 1, 2, 1])
    rows = np.array([[1, 2, 3],      # class 0: own label at rank 1
                     [2, 0, 3],      # class 0: at rank 2
                     [0, 1, 4],      # class 1: never within 3
                     [0, 4, 5],      # class 1: at rank 3
                     [0, 1, 2],      # class 2 has one image: left out
                     [3, -1, -1]])   # class 1: at rank 1, short list
    curve, left_out = cmc(labels, rows)
    assert left_out == 1 and curve.dtype == np.float64
    assert np.array_equal(curve, np.array([2, 3, 4]) / 5)
    curve, left_out = cmc(np.array([3, 4]), np.array([[1], [0]]))
    assert left_out == 2 and np.array_equal(curve, [0.0])
    with pytest.raises(ValueError, match="cmc"):
        cmc(labels, rows[:3])


def test_gallery_argument_errors_need_no_device(tmp_path):
    from facenet_amd.recognize import Gallery
    emb = io.unit_rows(6, 8, 1)
    with pytest.raises(ValueError, match="Undefined similarity metric 2"):
        Gallery(emb, metric=2, device="cpu")
    with pytest.raises(ValueError, match="2-D"):
        Gallery(emb[0], device="cpu")
    with pytest.raises(ValueError, match="multiple of 4"):
        Gallery(np.ones((3, 6), np.float32), device="cpu")
    with pytest.raises(ValueError, match="multiple of 4"):
        Gallery(np.ones((3, 516), np.float32), device="cpu")
    with pytest.raises(ValueError, match="labels must be 6 integers"):
        Gallery(emb, labels=[0, 1], device="cpu")
    with pytest.raises(ValueError, match="-1 is what an unidentified face gets"):
        Gallery(emb, labels=[0, 1, 2, 3, 4, -1], device="cpu")
    with pytest.raises(ValueError, match="names must cover every label"):
        Gallery(emb, labels=[0, 0, 1, 1, 2, 2], names=["a", "b"], device="cpu")
    with pytest.raises(ValueError, match="files must name 6 rows"):
        Gallery(emb, files=["x"], device="cpu")
    with pytest.raises(ValueError, match="h5py"):
        Gallery.from_file(tmp_path / "embeddings.h5")

    files = [f"/data/{cls}/{i}.png" for cls in ("ann", "bob", "cy") for i in range(2)]
    np.savez(tmp_path / "e.npz", embeddings=emb, labels=np.array([0, 0, 1, 1, 2, 2]), files=np.array(files))
    g = Gallery.from_file(tmp_path / "e.npz", device="cpu")
    assert (g.nrof_images, g.nrof_classes, g.length) == (6, 3, 8) and g.names == {0: "ann", 1: "bob", 2: "cy"}
    assert Gallery(emb, device="cpu").nrof_classes == 6
    for bad_k in (0, 65):
        with pytest.raises(ValueError, match=r"k must be in \[1, 64\]"):
            g.search(emb, k=bad_k)
    with pytest.raises(ValueError, match="embedding lengths differ: queries 12, gallery 8"):
        g.search(np.ones((2, 12), np.float32))
    with pytest.raises(ValueError, match="skip must be 6 integers"):
        g.search(emb, skip=[1, 2])
    with pytest.raises(ValueError, match="not both"):
        g.identify(emb, threshold=1.0, classifier=object())
    with pytest.raises(ValueError, match="FaceToFaceNormalizedEmbeddingsClassifier"):
        g.identify(emb, classifier=object())
    dist, rows = g.search(np.zeros((0, 8), np.float32), k=3)             # no launch: this gallery lives on the host
    assert dist.shape == (0, 3) and dist.dtype == np.float32 and rows.shape == (0, 3) and rows.dtype == np.int32
    assert g.identify(np.zeros((0, 8), np.float32)) == []


def test_app_options(tmp_path):
    from facenet_amd.apps import identify as app
    base = {"dataset": {"path": str(tmp_path / "photos")}, "gallery": {"path": str(tmp_path / "g.npz")}}
    c = app.load_options(overrides=base)
    assert c.file == tmp_path / "photos_model" / "identified.npz" and c.gallery.path == tmp_path / "g.npz"
    assert c.gallery.metric == 0 and c.identify.k == 1 and c.identify.threshold is None and c.identify.classifier is None
    assert c.image.size == 160 and c.image.margin == 0.14 and c.detector == "pypimtcnn"
    c = app.load_options(overrides=dict(base, model={"path": "~/models/best.npz"}, identify={"k": 5, "threshold": 1.1},
                                        gallery={"path": str(tmp_path / "g.npz"), "metric": 1}))
    assert c.file == tmp_path / "photos_best" / "identified.npz" and c.identify.k == 5 and c.identify.threshold == 1.1
    assert c.gallery.metric == 1
    with pytest.raises(ValueError, match="gallery.path is not specified"):
        app.load_options(overrides={"dataset": {"path": "x"}})
    with pytest.raises(ValueError, match="dataset.path is not specified"):
        app.load_options(overrides={"gallery": {"path": "g.npz"}})
    with pytest.raises(ValueError, match="not both"):
        app.load_options(overrides=dict(base, identify={"threshold": 1.0, "classifier": "c.npz"}))
    with pytest.raises(ValueError, match=r"identify.k must be an integer in \[1, 64\]"):
        app.load_options(overrides=dict(base, identify={"k": 65}))
    with pytest.raises(ValueError, match="Undefined similarity metric 3"):
        app.load_options(overrides=dict(base, gallery={"path": "g.npz", "metric": 3}))
    with pytest.raises(ValueError, match="must be an .npz"):
        app.load_options(overrides=dict(base, file="out.h5"))
    cfg = tmp_path / "x.yaml"
    cfg.write_text("dataset: {path: /d}\ngallery: {path: /g.npz}\nidentify: {classifier: /c.npz}\nfile: /o/who.npz\n")
    c = app.load_options(cfg)
    assert str(c.file) == "/o/who.npz" and str(c.identify.classifier) == "/c.npz" and c.identify.threshold is None
