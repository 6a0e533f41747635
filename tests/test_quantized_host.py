"""The quantised gallery without a device: the NumPy oracle (tests/quantized_oracle.py) against identify_oracle.search, the bound
of the certificate, the argument errors of Gallery.quantize / QuantizedGallery, the app's options and the C ABI's new entries."""
import ctypes as C

import numpy as np
import pytest

from tests import identify_oracle as io
from tests import quantized_oracle as qo

U = 2.0 ** -24


def one_hot(n, E, seed):
    x = np.zeros((n, E), dtype=np.float32)
    x[np.arange(n), np.random.default_rng(seed).integers(0, E, n)] = 1
    return x


@pytest.mark.parametrize("E", [4, 40, 128, 512])
def test_quantisation_rules(E):
    x = np.concatenate([io.unit_rows(30, E, E), one_hot(3, E, E + 1), np.zeros((1, E), np.float32)])
    x[1] *= np.float32(1 + 1e-3)
    x[2, 0] = -np.abs(x[2]).max() * 2                          # the maximum is a negative entry
    got = qo.quantize(x)
    codes = got["codes"].astype(np.int64)
    assert codes.shape == (34, qo.padded(E)) and np.abs(codes).max() == 127 and (codes[:, E:] == 0).all()
    assert (np.abs(codes[:-1]).max(axis=1) == 127).all()       # some |c| = 127 in every non-zero row
    assert (codes[-1] == 0).all() and got["scale"][-1] == 0 and got["rho"][-1] == 0 and got["norm"][-1] == 0
    assert codes[2, 0] == -127
    assert (got["rho"].astype(np.float64) >= got["rho64"]).all() and (got["norm"].astype(np.float64) >= got["norm64"]).all()
    assert (np.nextafter(got["rho"][:-1], np.float32(-np.inf)).astype(np.float64) < got["rho64"][:-1]).all()      # and the smallest such
    exact = np.linalg.norm(x.astype(np.float64) - got["scale"].astype(np.float64)[:, None] * codes[:, :E], axis=1)
    assert np.allclose(got["rho64"], exact, rtol=1e-12, atol=0) and np.allclose(got["norm64"], np.linalg.norm(x.astype(np.float64), axis=1), rtol=1e-12)


def test_codes_round_half_to_even():
    """m = 127 2^-8 and x_e = (j + 1/2) 2^-8: x 127 / m = j + 1/2 exactly, which goes to the even neighbour."""
    j = np.arange(0, 60)
    x = np.concatenate([[127.0], j + 0.5, -(j + 0.5)])[None, :] * 2.0 ** -8
    x = np.concatenate([x, np.zeros((1, 3))], axis=1).astype(np.float32)        # E = 124
    codes = qo.quantize(x)["codes"][0].astype(np.int64)
    even = np.where(j % 2 == 0, j, j + 1)
    assert codes[0] == 127 and np.array_equal(codes[1:61], even) and np.array_equal(codes[61:121], -even)


@pytest.mark.parametrize("E", [4, 40, 128, 512])
def test_the_bound_holds_for_every_pair(E):
    """|s^ - s_chain| <= B - 4 u: the first two terms of B bound |x.y - x^.y^|, the third the fp32 chain against x.y."""
    q = np.concatenate([io.unit_rows(12, E, 100 + E), one_hot(2, E, 7)])
    g = np.concatenate([io.unit_rows(40, E, 200 + E), one_hot(4, E, 8)])
    q[:6] *= np.linspace(1 - 1e-3, 1 + 1e-3, 6, dtype=np.float32)[:, None]
    g[:10] *= np.linspace(1 - 1e-3, 1 + 1e-3, 10, dtype=np.float32)[:, None]
    qq, gq = qo.quantize(q), qo.quantize(g)
    err = np.abs(qo.estimates(qq, gq).astype(np.float64) - io.chain_similarities(q, g).astype(np.float64))
    rho_max, norm_max = float(gq["rho"].max()), float(gq["norm"].max())
    B = np.array([qo.bound(float(r), float(n), rho_max, norm_max, E) for r, n in zip(qq["rho"], qq["norm"])])
    assert (err <= (B - 4 * U)[:, None]).all(), (err.max(), B.min())
    assert ((qq["norm"] + qq["rho"]).astype(np.float64) * (norm_max + rho_max) <= 1.05).all()       # inside the certificate's domain


def same_where_certified(got, ref):
    c = got["certified"]
    assert np.array_equal(got["rows"][c], ref["rows"][c])
    assert np.array_equal(got["dist"][c].view(np.uint32), ref["dist"][c].view(np.uint32))
    return int(c.sum())


def test_certified_queries_have_the_exhaustive_answer():
    """Soundness: wherever the oracle certifies a query, its result is identify_oracle.search's bit for bit."""
    q, g = io.unit_rows(20, 128, 1), io.unit_rows(500, 128, 2)
    got = qo.search(q, g, 5, 64)
    assert same_where_certified(got, io.search(q, g, 5, s=got["s"])) == 20                 # random rows: every query
    skip = np.arange(20) * 3
    got = qo.search(q, g, 5, 64, skip=skip)
    assert same_where_certified(got, io.search(q, g, 5, skip=skip, s=got["s"])) == 20 and (got["rows"] != skip[:, None]).all()

    pool = io.tie_pool(260, 3)
    q, g = pool[:8].copy(), pool[8:].copy()
    g[100], g[17], g[200] = q[0], q[0], q[1]
    got = qo.search(q, g, 3, 16)
    ref = io.search(q, g, 3, s=got["s"])
    assert ref["rows"][0, :2].tolist() == [17, 100]
    same_where_certified(got, ref)

    g = qo.near_duplicates(3, 40, 128, 5, spread=0.011)                                     # classes of 40 near-duplicates
    q = g[::4].copy()
    got = qo.search(q, g, 1, 16)
    n = same_where_certified(got, io.search(q, g, 1, s=got["s"]))
    assert 0 < n < len(q), n                                                                # some certified, some not


def test_shortlist_oracle_by_hand():
    x, c = qo.small_integer_codes(6, 64, 1)
    qq = qo.quantize(x)
    assert np.array_equal(qq["codes"].astype(np.int64), c) and (qq["scale"] == np.float32(2.0 ** -13)).all() and (qq["rho"] == 0).all()
    est = qo.estimates(qq, qq)
    assert np.array_equal(est.astype(np.float64), (c @ c.T) * 2.0 ** -26)
    keys = qo.shortlist_keys(est, 8, skip=np.arange(6))
    assert (keys[:, 5:] == qo.NONE).all() and ((keys[:, :5] & np.uint64(0xFFFFFFFF)) != np.arange(6, dtype=np.uint64)[:, None]).all()
    got = qo.search(x, x, 2, 8)
    assert got["certified"].all()                              # a shortlist that is not full holds every admissible row


def test_argument_errors_need_no_device():
    from facenet_amd import _lib
    from facenet_amd.ivf import IVFGallery
    from facenet_amd.recognize import Gallery, QuantizedGallery
    emb = io.unit_rows(6, 8, 1)
    gal = Gallery(emb, labels=[0, 0, 1, 1, 2, 2], names=["ann", "bob", "cy"], device="cpu")
    for bad in (0, 65, 2.5, True):
        with pytest.raises(ValueError, match=r"shortlist must be an integer in \[1, 64\]"):
            gal.quantize(bad)
    index = IVFGallery.from_assignment(gal, io.unit_rows(3, 8, 2), np.array([2, 0, 2, 0, 0, 2]))
    with pytest.raises(NotImplementedError, match="quantised inverted-file lists are not built"):
        index.quantize()
    qg = gal.quantize(16)
    assert isinstance(qg, QuantizedGallery) and qg.shortlist == 16 and qg.codes is None and qg.last_fallbacks == 0
    assert np.array_equal(qg.labels, gal.labels) and qg.names == gal.names and "shortlist: 16" in repr(qg)
    assert (qg.nrof_images, qg.nrof_classes, qg.length, qg.metric) == (6, 3, 8, 0)
    for bad_k in (0, 65):
        with pytest.raises(ValueError, match=r"k must be in \[1, 64\]"):
            qg.search(emb, k=bad_k)
    for bad in (2, 65, 4.0, True):
        with pytest.raises(ValueError, match=r"shortlist must be an integer in \[3, 64\]"):
            qg.search(emb, k=3, shortlist=bad)
        with pytest.raises(ValueError, match=r"shortlist must be an integer in \[3, 64\]"):
            qg.search_certified(emb, k=3, shortlist=bad)
        with pytest.raises(ValueError, match=r"shortlist must be an integer in \[3, 64\]"):
            qg.identify(emb, k=3, shortlist=bad)
        with pytest.raises(ValueError, match=r"shortlist must be an integer in \[3, 64\]"):
            qg.leave_one_out(3, shortlist=bad)
    with pytest.raises(ValueError, match="exact must be True or False"):
        qg.search(emb, exact=1)
    with pytest.raises(ValueError, match="embedding lengths differ: queries 12, gallery 8"):
        qg.search(np.ones((2, 12), np.float32))
    with pytest.raises(ValueError, match="skip must be 6 integers"):
        qg.search(emb, skip=[1, 2])
    with pytest.raises(ValueError, match="not both"):
        qg.identify(emb, threshold=1.0, classifier=object())
    with pytest.raises(_lib.FacenetHipError, match="no CPU fallback"):
        qg.search(emb)
    with pytest.raises(_lib.FacenetHipError, match="no CPU fallback"):
        qg.search_certified(emb)
    dist, rows = qg.search(np.zeros((0, 8), np.float32), k=3)
    assert dist.shape == (0, 3) and dist.dtype == np.float32 and rows.shape == (0, 3) and rows.dtype == np.int32
    dist, rows, certified = qg.search_certified(np.zeros((0, 8), np.float32), k=3)
    assert dist.shape == (0, 3) and certified.shape == (0,) and certified.dtype == bool
    assert qg.identify(np.zeros((0, 8), np.float32)) == []


def test_app_options(tmp_path):
    from click.testing import CliRunner
    from facenet_amd.apps import identify as app
    base = {"dataset": {"path": str(tmp_path / "photos")}, "gallery": {"path": str(tmp_path / "g.npz")}}
    c = app.load_options(overrides=base)
    assert c.identify.quantized is False and c.identify.shortlist is None          # off by default
    c = app.load_options(overrides=dict(base, identify={"quantized": True, "shortlist": 32, "k": 3}))
    assert (c.identify.quantized, c.identify.shortlist, c.identify.k) == (True, 32, 3)
    assert app.load_options(overrides=dict(base, identify={"quantized": True})).identify.shortlist is None
    for bad in (0, 2, 65, 1.5, True):
        with pytest.raises(ValueError, match=r"identify.shortlist must be an integer in \[identify.k, 64\]"):
            app.load_options(overrides=dict(base, identify={"quantized": True, "k": 3, "shortlist": bad}))
    for bad in (1, "yes", None):
        with pytest.raises(ValueError, match="identify.quantized must be true or false"):
            app.load_options(overrides=dict(base, identify={"quantized": bad}))
    with pytest.raises(ValueError, match="identify.shortlist needs identify.quantized"):
        app.load_options(overrides=dict(base, identify={"shortlist": 16}))
    with pytest.raises(ValueError, match="identify.quantized cannot be combined with identify.nlist"):
        app.load_options(overrides=dict(base, identify={"quantized": True, "nlist": 8}))
    seen = {}
    original = app.write_identified
    app.write_identified = lambda options: seen.update(quantized=options.identify.quantized, shortlist=options.identify.shortlist)
    try:
        cfg = tmp_path / "x.yaml"
        cfg.write_text(f"dataset: {{path: {tmp_path}/d}}\ngallery: {{path: {tmp_path}/g.npz}}\nidentify: {{k: 2}}\n")
        assert CliRunner().invoke(app.main, ["--config", str(cfg)]).exit_code == 0 and seen == {"quantized": False, "shortlist": None}
        result = CliRunner().invoke(app.main, ["--config", str(cfg), "--quantized", "--shortlist", "16"])
        assert result.exit_code == 0 and seen == {"quantized": True, "shortlist": 16}
        assert CliRunner().invoke(app.main, ["--config", str(cfg), "--shortlist", "16"]).exit_code != 0
        assert CliRunner().invoke(app.main, ["--config", str(cfg), "--quantized", "--nlist", "4"]).exit_code != 0
    finally:
        app.write_identified = original


def test_abi_exports_and_workspace_rules():
    from facenet_amd import _lib
    lib = _lib.load()
    for name in ("fn_quantize_rows", "fn_qgallery_search", "fn_qgallery_search_workspace"):
        assert name in _lib.EXPORTS and hasattr(lib, name)
    assert lib.fn_abi_version() == 1
    nbytes = C.c_longlong(-1)
    assert lib.fn_qgallery_search_workspace(70, 300, 5, 16, 64, C.byref(nbytes)) == 0 and nbytes.value == 5 * 70 * 16 * 8
    assert lib.fn_qgallery_search_workspace(70, 300, 5, 16, 1, C.byref(nbytes)) == 0 and nbytes.value == 5 * 70 * 16 * 8
    assert lib.fn_qgallery_search_workspace(16, 150, 7, 7, 128, C.byref(nbytes)) == 0 and nbytes.value == 2 * 4 * 16 * 7 * 8
    assert lib.fn_qgallery_search_workspace(17, 150, 1, 64, 0, C.byref(nbytes)) == 0 and nbytes.value == 17 * 64 * 8
    assert lib.fn_qgallery_search_workspace(5, 1100, 3, 9, 64, C.byref(nbytes)) == 0 and nbytes.value == (72 + 3) * 5 * 9 * 8      # + the groups
    assert lib.fn_qgallery_search_workspace(5, 1024, 3, 9, 64, C.byref(nbytes)) == 0 and nbytes.value == 64 * 5 * 9 * 8            # 64 lists: none
    for bad in ((0, 300, 5, 16, 0), (70, 0, 5, 16, 0), (70, 300, 0, 16, 0), (70, 300, 65, 65, 0), (70, 300, 5, 4, 0), (70, 300, 5, 65, 0),
                (70, 300, 5, 16, -1), (1, 2 ** 31 - 1, 1, 1, 64)):
        assert lib.fn_qgallery_search_workspace(*bad, C.byref(nbytes)) == -1 and lib.fn_last_error().decode() != ""
    assert lib.fn_qgallery_search_workspace(70, 300, 5, 4, 0, C.byref(nbytes)) == -1
    assert "shortlist must be in [k, 64]" in lib.fn_last_error().decode()
    assert lib.fn_qgallery_search_workspace(70, 300, 5, 16, 0, None) == -1 and "bad arguments" in lib.fn_last_error().decode()
    # the entries refuse their arguments before anything is launched: no device is needed for these
    assert lib.fn_quantize_rows(None, 1, 8, None, None, None, None, None) == -1 and "bad arguments" in lib.fn_last_error().decode()
    assert lib.fn_quantize_rows(None, 0, 8, None, None, None, None, None) == -1 and "N must be at least 1" in lib.fn_last_error().decode()
    for E in (0, 6, 516):
        assert lib.fn_quantize_rows(None, 1, E, None, None, None, None, None) == -1 and "multiple of 4" in lib.fn_last_error().decode()
