"""Open-set 1:N evaluation without a device: the NumPy oracle of fn_mate_search (tests/opensearch_oracle.py) against brute force in
fp64, the exact-tie pool, `IdentificationCurve.from_search` against sorting and counting, and every argument error of
`Gallery.mates`, `IdentificationCurve` and `identification_curve`."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

from tests import identify_oracle as io
from tests import opensearch_oracle as oo

CASES = ((8, 200, 32, 1), (5, 70, 128, 2), (3, 40, 512, 3))          # (Q, G, E, seed): 16 queries in all


def test_oracle_agrees_with_fp64_brute_force():
    """Where the fp64 distances of the best and the runner-up of a population are further apart than twice the fp32 chain's error
    bound (|d0 - d64| <= 2 gamma_E + 4 u: tests/test_identify_host.py), the oracle's nearest mate and nearest impostor ARE the
    fp64 ones, and so is the rank when no impostor lies within the bound of the mate."""
    left_out = total = 0
    u = 2.0 ** -24
    for (Q, G, E, seed) in CASES:
        q, g = io.unit_rows(Q, E, seed), io.unit_rows(G, E, 100 + seed)
        glabels = oo.ragged_labels([G // 4, G // 4, G // 8, 1, G - 2 * (G // 4) - G // 8 - 1], seed)
        qlabels = np.random.default_rng(seed).integers(0, 5, Q)
        skip = np.random.default_rng(50 + seed).integers(-1, G, Q)
        got = oo.mates(q, qlabels, g, glabels, skip=skip)
        bound = 2 * (E * u / (1 - E * u)) + 4 * u
        d64 = 2 * (1 - np.clip(q.astype(np.float64) @ g.astype(np.float64).T, -1, 1))
        for i in range(Q):
            total += 1
            ok = np.arange(G) != skip[i]
            pops = [np.nonzero(ok & (glabels == qlabels[i]))[0], np.nonzero(ok & (glabels != qlabels[i]))[0]]
            srt = [p[np.argsort(d64[i, p], kind="stable")] for p in pops]
            gaps = [d64[i, s[1]] - d64[i, s[0]] for s in srt if len(s) > 1]
            assert len(srt[0]) and len(srt[1])
            mate64 = d64[i, srt[0][0]]
            near = np.abs(d64[i, pops[1]] - mate64).min()                    # an impostor this near the mate could swap places
            if min(gaps) <= 2 * bound or near <= 2 * bound:
                left_out += 1
                continue
            assert got["rows"][i].tolist() == [srt[0][0], srt[1][0]], (Q, G, E, i)
            assert np.abs(got["dist"][i].astype(np.float64) - d64[i, got["rows"][i]]).max() <= bound
            assert got["ranks"][i] == np.count_nonzero(d64[i, pops[1]] < mate64)
    assert total == 16 and left_out == 0          # the share of cases the gap condition leaves out: 0 / 16 for these seeds


def test_oracle_agrees_with_the_search_oracle():
    """The full ordering of identify_oracle.search holds the same mate, impostor and rank."""
    x, labels = io.unit_rows(40, 16, 7), oo.ragged_labels([9, 1, 14, 5, 11], 3)
    got = oo.leave_one_out(x, labels, metric=1)
    full = io.search(x, x, 39, metric=1, skip=np.arange(40))
    for i in range(40):
        same = labels[full["rows"][i]] == labels[i]
        first_mate = int(np.argmax(same)) if same.any() else -1
        assert got["ranks"][i] == first_mate
        assert got["rows"][i, 1] == full["rows"][i][np.argmax(~same)] and got["dist"][i, 1] == full["dist"][i][np.argmax(~same)]
        assert got["rows"][i, 0] == (full["rows"][i][first_mate] if first_mate >= 0 else -1)
    assert got["ranks"][labels == 1].tolist() == [-1] and np.isposinf(got["dist"][labels == 1, 0]).all()
    absent = oo.mates(x[:3], [-1, labels[1], -1], x, labels)             # -1: every row an impostor, the row itself included
    assert absent["ranks"].tolist() == [-1, 0, -1] and absent["rows"][0].tolist() == [-1, 0] and absent["rows"][1, 0] == 1


def test_tie_pool_equal_distances_go_to_the_lower_row():
    pool = io.tie_pool(40, 5)
    g, labels = pool[4:].copy(), np.arange(36) % 3
    q, qlabels = pool[:4].copy(), np.array([0, 1, 2, 0])
    g[9] = g[21] = q[0]            # label 0: two mates of query 0 at distance 0
    g[10] = g[13] = q[0]           # label 1: two impostors of query 0 at distance 0, one of them before mate 21
    got = oo.mates(q, qlabels, g, labels)
    assert got["rows"][0].tolist() == [9, 10] and got["dist"][0].tolist() == [0.0, 0.0]
    assert got["ranks"][0] == 0                                            # impostor keys at d0 = 0: rows 10 and 13, both above row 9
    got = oo.mates(q, qlabels, g, labels, skip=[9, -1, -1, -1])
    assert got["rows"][0].tolist() == [21, 10] and got["ranks"][0] == 2    # rows 10 and 13 precede row 21


# ---- the curve --------------------------------------------------------------------------------------------------------------------
def _scores(seed, n=60):
    """Mate / impostor distances on a coarse grid (ties in numbers), ranks consistent with them, a few probes without a mate."""
    rng = np.random.default_rng(seed)
    mate = (rng.integers(0, 24, n) / 16).astype(np.float32)
    imp = (rng.integers(4, 40, n) / 16).astype(np.float32)
    ranks = np.where(imp < mate, rng.integers(1, 5, n), 0).astype(np.int32)
    none = rng.random(n) < 0.15
    mate[none], ranks[none] = np.inf, -1
    return mate, imp, ranks, rng.integers(0, n, n).astype(np.int32)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_from_search_counts_like_sorting(seed):
    from facenet_amd.statistics import IdentificationCurve
    mate, imp, ranks, rows = _scores(seed)
    curve = IdentificationCurve.from_search(mate, imp, ranks, impostor_rows=rows)
    M, N = int((ranks >= 0).sum()), len(imp)
    assert (curve.nrof_mated, curve.nrof_nonmated, curve.nrof_probes) == (M, N, 60)
    fpirs = [0.0, 1 / N, 0.05, 0.1, 0.5, 1 - 1e-9, 1.0]
    for rank in (1, 3):
        got = curve.fnir_at_fpir(fpirs, rank=rank)
        want = oo.fnir_at_fpir(mate, imp, ranks, fpirs, rank=rank)
        for g, w in zip(got, want):
            assert {k: g[k] for k in w} == w and g["rank"] == rank
            m = int(Fraction(w["fpir_target"]) * N)
            assert g["false_positives"] <= m or g["threshold"] == float("inf")
        assert got[0]["threshold"] == float(np.sort(imp)[0]) and got[0]["false_positives"] == 0          # f = 0: below every impostor
        assert got[-1]["threshold"] == float("inf") and got[-1]["false_positives"] == N and got[-1]["fpir"] == 1.0
        assert got[-1]["hits"] == int(((ranks >= 0) & (ranks < rank)).sum())
        assert any(g["false_positives"] < int(Fraction(g["fpir_target"]) * N) for g in got[:-1])          # ties at a threshold exist
    assert curve.fnir_at_fpir([0.5], rank=3)[0]["hits"] >= curve.fnir_at_fpir([0.5], rank=1)[0]["hits"]
    for t in (0.0, 0.5, float(imp[3]), float(mate[np.isfinite(mate)][0]), 4.0, float("inf")):
        for rank in (1, 2):
            fp, hits = oo.counts_at(mate, imp, ranks, t, rank)
            got = curve.dir_at(t, rank=rank)
            assert (got["false_positives"], got["hits"], got["fpir"], got["dir"], got["fnir"]) == (fp, hits, fp / N, hits / M, 1 - hits / M)
    for k in (1, 2, 5, 200):
        got, left_out = curve.cmc(k)
        want, want_left = oo.cmc(ranks, k)
        assert got.dtype == np.float64 and got.shape == (k,) and np.array_equal(got, want) and left_out == want_left == 60 - M
    assert curve.cmc(200)[0][-1] == 1.0
    assert curve.mislabelled() == oo.mislabelled(mate, imp, rows, ranks) and len(curve.mislabelled()) == int((ranks > 0).sum()) > 0
    d = curve.dict()
    assert d["nrof_mated"] == M and d["rank1"] == curve.cmc(1)[0][0] and d["nrof_mislabelled"] == len(curve.mislabelled())
    text = str(curve)
    assert text.startswith("IdentificationCurve\nmetric: 0\n\nmated searches: {}\nnon-mated searches: {}\n".format(M, N))
    assert text.count("FNIR @ FPIR = ") == len(d["fnir_at_fpir"]) and "FNIR @ FPIR = 0.05 (rank 3)\n" in text


def test_cmc_equals_statistics_cmc_on_the_search_rows():
    from facenet_amd.statistics import IdentificationCurve, cmc
    x, labels = io.unit_rows(90, 16, 11), oo.ragged_labels([30, 1, 25, 2, 1, 31], 4)
    found = oo.leave_one_out(x, labels)
    curve = IdentificationCurve.from_search(found["dist"][:, 0], found["dist"][:, 1], found["ranks"], impostor_rows=found["rows"][:, 1])
    for k in (1, 7, 64):
        want, want_left = cmc(labels, io.search(x, x, k, skip=np.arange(90), s=found["s"])["rows"])
        got, left_out = curve.cmc(k)
        assert np.array_equal(got, want) and left_out == want_left == 2
    assert curve.cmc(64)[0][-1] < 1.0 and curve.cmc(89)[0][-1] == 1.0       # a class of 31 hides mates beyond rank 64... the curve goes on


def test_argument_errors_need_no_device():
    from facenet_amd.recognize import Gallery, MateSearch
    from facenet_amd.statistics import IdentificationCurve
    emb = io.unit_rows(6, 8, 1)
    g = Gallery(emb, labels=[5, 5, 9, 9, 2 ** 40, 7], device="cpu")
    with pytest.raises(ValueError, match="2-D"):
        g.mates(emb[0], [0])
    with pytest.raises(ValueError, match="embedding lengths differ: queries 12, gallery 8"):
        g.mates(np.ones((2, 12), np.float32), [0, 0])
    with pytest.raises(ValueError, match="labels must be 6 integers"):
        g.mates(emb, [5, 9])
    with pytest.raises(ValueError, match="labels must be 6 integers"):
        g.mates(emb, np.ones(6))
    with pytest.raises(ValueError, match="must not be below -1"):
        g.mates(emb, [5, 5, 9, -2, 7, 7])
    with pytest.raises(ValueError, match="skip must be 6 integers"):
        g.mates(emb, [5, 5, 9, 9, 7, 7], skip=[1, 2])
    assert g.query_codes([5, 9, 2 ** 40, 7, -1, 6, 2 ** 41], 7).tolist() == [0, 2, 3, 1, -1, -1, -1]
    assert g.query_codes([], 0).shape == (0,)
    from facenet_amd._lib import FacenetHipError
    with pytest.raises(FacenetHipError, match="Gallery.mates runs fn_mate_search"):
        g.mates(emb, [5, 5, 9, 9, 7, 7])                                  # every check passed: this gallery lives on the host
    for ranks in (True, False):
        out = g.mates(np.zeros((0, 8), np.float32), [], ranks=ranks)      # no launch
        assert isinstance(out, MateSearch) and out.mate_dist.shape == out.impostor_rows.shape == (0,)
        assert out.mate_dist.dtype == np.float32 and out.mate_rows.dtype == np.int32
        assert (out.ranks is None) == (not ranks) and (out.ranks is None or out.ranks.shape == (0,))

    with pytest.raises(ValueError, match="Undefined similarity metric 2"):
        IdentificationCurve(emb, [0, 0, 1, 1, 2, 2], metric=2, device="cpu")
    with pytest.raises(ValueError, match="mated and non-mated searches, got 0 and 6"):
        IdentificationCurve(emb, [0, 1, 2, 3, 4, 5], device="cpu")        # before any launch: no device here
    with pytest.raises(ValueError, match="mated and non-mated searches, got 6 and 0"):
        IdentificationCurve(emb, [3, 3, 3, 3, 3, 3], device="cpu")
    with pytest.raises(ValueError, match="Undefined similarity metric 3"):
        IdentificationCurve.from_search([0.1], [0.2], [0], metric=3)
    with pytest.raises(ValueError, match="equal length"):
        IdentificationCurve.from_search([0.1, 0.2], [0.2], [0])
    with pytest.raises(ValueError, match="equal length"):
        IdentificationCurve.from_search([0.1], [0.2], [0.0])
    with pytest.raises(ValueError, match="got 0 and 1"):
        IdentificationCurve.from_search([np.inf], [0.2], [-1])
    with pytest.raises(ValueError, match="got 1 and 0"):
        IdentificationCurve.from_search([0.1], [np.inf], [0])
    curve = IdentificationCurve.from_search([0.1, 0.3], [0.2, 0.25], [0, 1])
    for bad in ([0.1, 0.01], [-1e-9], [0.5, 1.0000001], [float("nan")]):
        with pytest.raises(ValueError, match="false-positive identification rates"):
            curve.fnir_at_fpir(bad)
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="rank must be an integer of at least 1"):
            curve.fnir_at_fpir([0.1], rank=bad)
        with pytest.raises(ValueError, match="rank must be an integer of at least 1"):
            curve.dir_at(0.5, rank=bad)
        with pytest.raises(ValueError, match="k must be an integer of at least 1"):
            curve.cmc(bad)
    with pytest.raises(ValueError, match="NaN"):
        curve.dir_at(float("nan"))
    assert curve.mislabelled() == [(1, -1, float(np.float32(0.3)), 0.25)]


def test_the_config_key_is_off_by_default(tmp_path):
    from facenet_amd import statistics as st
    from facenet_amd.apps.validate import load_options
    opt = load_options(overrides={"model": {"path": str(tmp_path)}})
    assert st.identification_curve(None, None, opt.validate) is None                  # nothing is looked at
    opt = load_options(overrides={"model": {"path": str(tmp_path)}, "validate": {"fpir_targets": None}})
    assert st.identification_curve(None, None, opt.validate) is None
    emb = io.unit_rows(4, 8, 2)
    opt = load_options(overrides={"model": {"path": str(tmp_path)}, "validate": {"fpir_targets": [0.01, 2.0]}})
    with pytest.raises(ValueError, match="false-positive identification rates must lie in"):
        st.identification_curve(emb, [0, 0, 1, 1], opt.validate, device="cpu")
    opt = load_options(overrides={"model": {"path": str(tmp_path)}, "validate": {"fpir_targets": [0.01], "fpir_rank": 0}})
    with pytest.raises(ValueError, match="rank must be an integer of at least 1"):
        st.identification_curve(emb, [0, 0, 1, 1], opt.validate, device="cpu")
    opt = load_options(overrides={"model": {"path": str(tmp_path)}, "validate": {"fpir_targets": [0.01], "metric": 5}})
    with pytest.raises(ValueError, match="Undefined similarity metric 5"):
        st.identification_curve(emb, [0, 0, 1, 1], opt.validate, device="cpu")
    opt = load_options(overrides={"model": {"path": str(tmp_path)}, "validate": {"fpir_targets": [0.01]}})
    with pytest.raises(ValueError, match="mated and non-mated searches, got 0 and 4"):
        st.identification_curve(emb, [0, 1, 2, 3], opt.validate, device="cpu")


def test_callback_appends_the_curve_only_with_the_key(tmp_path, monkeypatch):
    """The wiring with a stub in place of the curve (tests/test_gpu_opensearch.py runs the real one): with the key unset the
    report file and the log are what they are without this feature."""
    from facenet_amd import callbacks
    from facenet_amd import statistics as st
    from facenet_amd.config import Config
    data = [(np.ones((3, 2, 2, 3), np.uint8), np.array([0, 0, 1]))]

    class Model:
        def __init__(self, path):
            self.path = path

        def __call__(self, images):
            return np.asarray(images, np.float32).reshape(len(images), -1)[:, :2]

    class Report:
        dict = {"stub": 1}

        def __init__(self, embeddings, labels, config):
            pass

        def __repr__(self):
            return "stub report\n"

        def write_report(self, file):
            with open(file, "at") as f:
                f.write(str(self))

    monkeypatch.setattr(st, "verification_curve", lambda e, l, config, device="cuda": None if isinstance(config.far_targets, Config) else "stub far\n")
    monkeypatch.setattr(st, "identification_curve",
                        lambda e, l, config, device="cuda": None if isinstance(config.fpir_targets, Config) else "stub fpir {}\n".format(config.fpir_targets))
    base = {"metric": 0, "nrof_folds": 2, "far_target": 1e-3}
    sep = 64 * "-" + "\n"
    for k, (extra, want) in enumerate((({}, "stub report\n"), ({"fpir_targets": [0.1]}, "stub report\n" + sep + "stub fpir [0.1]\n"),
                                       ({"far_targets": [0.1], "fpir_targets": [0.1]}, "stub report\n" + sep + "stub far\n" + sep + "stub fpir [0.1]\n"))):
        lines = []
        cb = callbacks.ValidateCallback(Model(tmp_path / f"run{k}"), data, 1, 1, Config({"validate": dict(base, **extra)}),
                                        log=lambda s: lines.append(str(s)), statistic=Report)
        report = cb.on_epoch_end(0)
        assert (tmp_path / f"run{k}" / "report.txt").read_text() == want
        assert hasattr(report, "identification") == bool(extra) and [l for l in lines if l.startswith("stub")] == want.replace(sep, "").splitlines(True)


def test_library_exports_and_workspace_rules():
    from facenet_amd import _lib
    assert "fn_mate_search" in _lib.EXPORTS and "fn_mate_search_workspace" in _lib.EXPORTS
    lib = _lib.load()
    assert hasattr(lib, "fn_mate_search") and hasattr(lib, "fn_mate_search_workspace") and lib.fn_abi_version() == 1
    nbytes = C.c_longlong(-1)
    for bad in ((0, 3, 0), (2, 0, 0), (2, 3, -1), (-1, 3, 0)):
        assert lib.fn_mate_search_workspace(*bad, C.byref(nbytes)) == -1 and lib.fn_last_error().decode() != "" and nbytes.value == -1
    assert lib.fn_mate_search_workspace(2, 3, 0, None) == -1 and "bad arguments" in lib.fn_last_error().decode()
    assert lib.fn_mate_search_workspace(3, 10 ** 9, 64, C.byref(nbytes)) == -1 and "at most 65535" in lib.fn_last_error().decode()
    per_slab = lambda Q: Q * (2 * 8 + 4)        # two 64-bit keys and one count per (slab, query); then one mate key per query
    for Q, G, slab_rows, slabs in ((70, 300, 64, 5), (70, 300, 1, 5), (70, 300, 0, 1), (70, 300, 320, 1), (1, 1, 0, 1), (26495, 26495, 0, 20),
                                   (5, 2 ** 31 - 1, 2 ** 30, 2)):
        assert lib.fn_mate_search_workspace(Q, G, slab_rows, C.byref(nbytes)) == 0
        assert nbytes.value == slabs * per_slab(Q) + 8 * Q, (Q, G, slab_rows)
