"""Candidate lists of identities without a device: the NumPy oracle (tests/candidates_oracle.py) against a direct loop and
against identify_oracle.search, the argument errors of Gallery.candidates / templates, the IVFGallery refusals, the app's options
and output arrays, and the C ABI's new entries."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import candidates_oracle as co
from tests import identify_oracle as io


def loop_candidates(s, labels, k, skip=None):
    """The definition, one pair at a time: per label the (d0, row)-smallest admissible row, then the k smallest of those."""
    _, d0 = io.distances(s)
    out = []
    for q in range(s.shape[0]):
        best = {}
        for g in range(s.shape[1]):
            if skip is not None and skip[q] == g:
                continue
            here = (float(d0[q, g]), g)
            if labels[g] not in best or here < best[labels[g]]:
                best[labels[g]] = here
        ranked = sorted((v, c) for c, v in best.items())[:k]
        out.append([(g, c, d) for (d, g), c in ranked])
    return out


def test_oracle_against_a_direct_loop():
    q, g = io.unit_rows(7, 12, 1), io.unit_rows(30, 12, 2)
    g[11] = g[3]                                               # equal distances inside one identity and between two
    g[20] = g[3]
    labels = np.array([5, 5, 9, 2, 2, 2, 7, 7, 7, 7, 0, 2, 3, 3, 9, 9, 9, 4, 4, 40, 41, 5, 5, 5, 6, 6, 1, 1, 1, 8])
    skip = np.array([3, -1, 10, 29, 0, -1, 19])
    s = io.chain_similarities(q, g)
    for k in (1, 4, 12, 20):
        for sk in (None, skip):
            got = co.candidates(q, g, labels, k, skip=sk, s=s)
            want = loop_candidates(s, labels, k, sk)
            for i, row in enumerate(want):
                n = len(row)
                assert got["rows"][i, :n].tolist() == [r for r, _, _ in row] and got["labels"][i, :n].tolist() == [c for _, c, _ in row]
                assert got["dist"][i, :n].tolist() == [d for _, _, d in row]
                assert (got["rows"][i, n:] == -1).all() and (got["labels"][i, n:] == -1).all() and np.isposinf(got["dist"][i, n:]).all()
                assert len(set(got["labels"][i, :n].tolist())) == n
    assert got["rows"].shape == (7, 20) and (got["rows"][:, 12:] == -1).all()           # 12 identities, one of them skipped away for query 6
    assert got["rows"][6, 11] == -1 and got["rows"][0, 11] >= 0
    ranks = co.identity_ranks(q, labels[:7], g, labels, skip=skip, s=s)
    wide = co.candidates(q, g, labels, 12, skip=skip, s=s)["labels"]
    assert ranks.tolist() == [int(np.nonzero(wide[i] == labels[i])[0][0]) for i in range(7)]
    assert co.identity_ranks(q[:1], [77], g, labels, s=s[:1]).tolist() == [-1]


def test_every_row_its_own_identity_is_the_search():
    q, g = io.unit_rows(5, 16, 3), io.unit_rows(40, 16, 4)
    skip = np.array([0, 7, -1, 39, 12])
    for metric in (0, 1):
        for k in (1, 7, 45):
            got, want = co.candidates(q, g, np.arange(40), k, metric=metric, skip=skip), io.search(q, g, k, metric=metric, skip=skip)
            assert np.array_equal(got["rows"], want["rows"]) and np.array_equal(got["dist"], want["dist"])
            assert np.array_equal(got["labels"], want["rows"])


def test_argument_errors_need_no_device():
    from facenet_amd import _lib
    from facenet_amd.ivf import IVFGallery
    from facenet_amd.recognize import Gallery
    emb = io.unit_rows(6, 8, 1)
    gal = Gallery(emb, labels=[4, 4, 1, 1, 9, 9], names={1: "ann", 4: "bob", 9: "cy"}, device="cpu")
    for bad_k in (0, 65):
        with pytest.raises(ValueError, match=r"k must be in \[1, 64\]"):
            gal.candidates(emb, k=bad_k)
        with pytest.raises(ValueError, match=r"k must be in \[1, 64\]"):
            gal.leave_one_out_candidates(bad_k)
        with pytest.raises(ValueError, match=r"k must be in \[1, 64\]"):
            gal.identify_candidates(emb, bad_k)
    with pytest.raises(ValueError, match="queries must be a 2-D"):
        gal.candidates(np.ones(8, np.float32))
    with pytest.raises(ValueError, match="embedding lengths differ: queries 12, gallery 8"):
        gal.candidates(np.ones((2, 12), np.float32))
    with pytest.raises(ValueError, match="skip must be 6 integers"):
        gal.candidates(emb, skip=[1, 2])
    with pytest.raises(ValueError, match="skip must be 6 integers"):
        gal.candidates(emb, skip=np.zeros(6))
    with pytest.raises(ValueError, match="not both"):
        gal.identify_candidates(emb, 2, threshold=1.0, classifier=object())
    with pytest.raises(ValueError, match="labels must not be negative"):
        Gallery(emb, labels=[0, 0, 1, -1, 2, 2], device="cpu")
    for call in (lambda: gal.candidates(emb, k=2), lambda: gal.leave_one_out_candidates(2), lambda: gal.identify_candidates(emb, 2),
                 gal.templates):
        with pytest.raises(_lib.FacenetHipError, match="no CPU fallback"):
            call()
    dist, rows, labels = gal.candidates(np.zeros((0, 8), np.float32), k=3)                # Q = 0: nothing needs a device
    assert dist.shape == rows.shape == labels.shape == (0, 3)
    assert (dist.dtype, rows.dtype, labels.dtype) == (np.float32, np.int32, np.int64)
    dist, rows, labels = gal.candidates(torch.zeros((0, 8)), k=3)
    assert torch.is_tensor(dist) and tuple(labels.shape) == (0, 3) and labels.dtype == torch.int64
    assert gal.identify_candidates(np.zeros((0, 8), np.float32), 3) == []
    index = IVFGallery.from_assignment(gal, io.unit_rows(3, 8, 2), np.array([2, 0, 2, 0, 0, 2]))
    for call in (lambda: index.candidates(emb, k=2), lambda: index.leave_one_out_candidates(2), lambda: index.identify_candidates(emb, 2),
                 index.templates):
        with pytest.raises(NotImplementedError, match="run this on the Gallery it was built from"):
            call()
    qg = gal.quantize(16)                                      # keeps the fp32 rows in order: the exhaustive path, unchanged
    assert type(qg).candidates is Gallery.candidates and type(qg).templates is Gallery.templates


def test_app_options(tmp_path):
    from click.testing import CliRunner
    from facenet_amd.apps import identify as app
    base = {"dataset": {"path": str(tmp_path / "photos")}, "gallery": {"path": str(tmp_path / "g.npz")}}
    c = app.load_options(overrides=base)
    assert c.identify.candidates is None and c.identify.templates is False                # off by default
    c = app.load_options(overrides=dict(base, identify={"candidates": 5, "templates": True, "k": 3}))
    assert (c.identify.candidates, c.identify.templates, c.identify.k) == (5, True, 3)
    assert app.load_options(overrides=dict(base, identify={"candidates": 64, "quantized": True})).identify.candidates == 64
    for bad in (0, 65, 2.5, True, "5"):
        with pytest.raises(ValueError, match=r"identify.candidates must be an integer in \[1, 64\]"):
            app.load_options(overrides=dict(base, identify={"candidates": bad}))
    for bad in (1, "yes", None):
        with pytest.raises(ValueError, match="identify.templates must be true or false"):
            app.load_options(overrides=dict(base, identify={"templates": bad}))
    with pytest.raises(ValueError, match="identify.templates cannot be combined with identify.nlist or identify.quantized"):
        app.load_options(overrides=dict(base, identify={"templates": True, "nlist": 8}))
    with pytest.raises(ValueError, match="identify.templates cannot be combined with identify.nlist or identify.quantized"):
        app.load_options(overrides=dict(base, identify={"templates": True, "quantized": True}))
    with pytest.raises(ValueError, match="identify.candidates cannot be combined with identify.nlist"):
        app.load_options(overrides=dict(base, identify={"candidates": 3, "nlist": 8}))
    seen = {}
    original = app.write_identified
    app.write_identified = lambda options: seen.update(candidates=options.identify.candidates, templates=options.identify.templates)
    try:
        cfg = tmp_path / "x.yaml"
        cfg.write_text(f"dataset: {{path: {tmp_path}/d}}\ngallery: {{path: {tmp_path}/g.npz}}\nidentify: {{k: 2}}\n")
        assert CliRunner().invoke(app.main, ["--config", str(cfg)]).exit_code == 0 and seen == {"candidates": None, "templates": False}
        result = CliRunner().invoke(app.main, ["--config", str(cfg), "--candidates", "5", "--templates"])
        assert result.exit_code == 0 and seen == {"candidates": 5, "templates": True}
        assert CliRunner().invoke(app.main, ["--config", str(cfg), "--candidates", "65"]).exit_code != 0
        assert CliRunner().invoke(app.main, ["--config", str(cfg), "--templates", "--nlist", "4"]).exit_code != 0
    finally:
        app.write_identified = original


class FakeGallery:
    """What write_identified asks of a gallery, answered on the host: every face's nearest rows are 0, 1, ..."""

    def __init__(self):
        self.calls = []

    def __repr__(self):
        return "FakeGallery"

    def search(self, emb, k=1):
        self.calls.append(("search", k))
        n = emb.shape[0]
        return torch.arange(k, dtype=torch.float32).repeat(n, 1), torch.arange(k, dtype=torch.int32).repeat(n, 1)

    def candidates(self, emb, k=1):
        self.calls.append(("candidates", k))
        n = emb.shape[0]
        return (torch.arange(k, dtype=torch.float32).repeat(n, 1), 10 * torch.arange(k, dtype=torch.int32).repeat(n, 1),
                100 + torch.arange(k, dtype=torch.int64).repeat(n, 1))

    def who(self, distance, row, threshold=None):
        return 100 + int(row), "ann", float(distance), int(row)


def test_app_output_arrays(tmp_path):
    """Both keys unset: exactly today's arrays and log lines.  identify.candidates adds its three arrays and nothing else."""
    from PIL import Image
    from facenet_amd.apps import identify as app
    (tmp_path / "photos" / "ann").mkdir(parents=True)
    for name in ("a.png", "b.png"):
        Image.fromarray(np.zeros((8, 8, 3), np.uint8)).save(tmp_path / "photos" / "ann" / name)
    box = SimpleNamespace(left=1, top=2, width=3, height=4, confidence=0.5)
    pipeline = SimpleNamespace(detector=SimpleNamespace(mode="RGB"), crops=lambda pixels: ([box, box], "crops"),
                               embed_device=lambda crops: torch.zeros((2, 8)))
    today = {"files", "face", "boxes", "confidence", "labels", "names", "distances", "rows"}
    logs = {}
    for key, identify in (("plain", {"k": 2}), ("wide", {"k": 2, "candidates": 3})):
        options = app.load_options(overrides={"dataset": {"path": str(tmp_path / "photos")}, "gallery": {"path": str(tmp_path / "g.npz")},
                                              "identify": identify, "file": str(tmp_path / f"{key}.npz")})
        gallery, lines = FakeGallery(), []
        app.write_identified(options, pipeline=pipeline, gallery=gallery, log=lambda *a: lines.append(" ".join(str(x) for x in a)))
        logs[key] = [line.replace(f"{key}.npz", "out.npz") for line in lines]
        with np.load(tmp_path / f"{key}.npz") as f:
            assert set(f.files) == (today if key == "plain" else today | {"candidate_labels", "candidate_distances", "candidate_rows"})
            assert f["rows"].shape == (4, 2) and f["labels"].tolist() == [100] * 4
            if key == "wide":
                assert f["candidate_labels"].dtype == np.int64 and f["candidate_labels"].tolist() == [[100, 101, 102]] * 4
                assert f["candidate_distances"].dtype == np.float32 and f["candidate_distances"].tolist() == [[0.0, 1.0, 2.0]] * 4
                assert f["candidate_rows"].dtype == np.int32 and f["candidate_rows"].tolist() == [[0, 10, 20]] * 4
        assert gallery.calls == ([("search", 2)] * 2 if key == "plain" else [("search", 2), ("candidates", 3)] * 2)
    assert logs["plain"] == logs["wide"] and sum("face" in line and "distance" in line for line in logs["plain"]) == 4


def test_abi_exports_and_workspace_rules():
    from facenet_amd import _lib
    lib = _lib.load()
    for name in ("fn_gallery_candidates", "fn_gallery_candidates_workspace"):
        assert name in _lib.EXPORTS and hasattr(lib, name)
    assert lib.fn_abi_version() == 1
    nbytes = C.c_longlong(-1)
    assert lib.fn_gallery_candidates_workspace(70, 300, 5, 64, C.byref(nbytes)) == 0 and nbytes.value == 5 * 70 * 5 * 8
    assert lib.fn_gallery_candidates_workspace(70, 300, 5, 1, C.byref(nbytes)) == 0 and nbytes.value == 5 * 70 * 5 * 8
    assert lib.fn_gallery_candidates_workspace(16, 150, 7, 128, C.byref(nbytes)) == 0 and nbytes.value == 2 * 4 * 16 * 7 * 8
    assert lib.fn_gallery_candidates_workspace(17, 150, 64, 0, C.byref(nbytes)) == 0 and nbytes.value == 17 * 64 * 8
    for bad in ((0, 300, 5, 0), (70, 0, 5, 0), (70, 300, 0, 0), (70, 300, 65, 0), (70, 300, 5, -1)):
        assert lib.fn_gallery_candidates_workspace(*bad, C.byref(nbytes)) == -1 and lib.fn_last_error().decode() != ""
    assert lib.fn_gallery_candidates_workspace(70, 300, 5, 0, None) == -1
