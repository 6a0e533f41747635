"""fn_quantize_rows / fn_qgallery_search / QuantizedGallery on the MI355X against the NumPy oracle (tests/quantized_oracle.py):
codes, scales, norms, shortlist keys, rows, metric-0 distances and certificates bit for bit, metric-1 distances within the 4-ulp
acosf rule of tests/test_gpu_identify.py, and the public search against Gallery.search on the device.  Output buffers are
over-allocated and pre-filled, so a write past an output is seen."""
import ctypes as C
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from facenet_amd import _lib
from facenet_amd.statistics import _decode_ord
from tests import identify_oracle as io
from tests import quantized_oracle as qo

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 7                      # extra words behind every output buffer
FILL_F, FILL_I, FILL_B = -77.0, -77, 0x5A


def _dev(a, dtype):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def gpu_quantize(x):
    """One fn_quantize_rows call -> dict(codes [N, Ep], scale, rho, norm); the guard words are checked here."""
    N, E = x.shape
    Ep = qo.padded(E)
    codes = torch.full((N * Ep + 16,), FILL_B, dtype=torch.int8, device=DEV)
    scale, rho, norm = (torch.full((N + GUARD,), FILL_F, dtype=torch.float32, device=DEV) for _ in range(3))
    xd = _dev(x, np.float32)
    rc = _lib.load().fn_quantize_rows(_ptr(xd), N, E, _ptr(codes), _ptr(scale), _ptr(rho), _ptr(norm), _stream())
    torch.cuda.synchronize()
    assert rc == 0, _lib.load().fn_last_error().decode()
    out = {"codes": codes.cpu().numpy(), "scale": scale.cpu().numpy(), "rho": rho.cpu().numpy(), "norm": norm.cpu().numpy()}
    assert (out["codes"][N * Ep:] == FILL_B).all()
    for name in ("scale", "rho", "norm"):
        assert (out[name][N:] == FILL_F).all()
        out[name] = out[name][:N]
    out["codes"] = out["codes"][:N * Ep].reshape(N, Ep)
    return out


def same_quantisation(got, ref):
    assert np.array_equal(got["codes"], ref["codes"])
    for name in ("scale", "rho", "norm"):
        assert np.array_equal(got[name].view(np.uint32), ref[name].view(np.uint32)), name


def gpu_qsearch(q, g, k, R, metric=0, skip=None, slab_rows=0, want_keys=True, want_range=True):
    """One fn_qgallery_search call on the oracle's quantised tables -> dict(rc, dist, rows, certified, keys, range)."""
    lib = _lib.load()
    Q, G, E = q.shape[0], g.shape[0], q.shape[1]
    qq, gq = qo.quantize(q), qo.quantize(g)
    nbytes = C.c_longlong(-1)
    rc = lib.fn_qgallery_search_workspace(Q, G, k, R, slab_rows, C.byref(nbytes))
    assert rc == 0 and nbytes.value >= Q * R * 8 and nbytes.value % (Q * R * 8) == 0
    ws = torch.full((nbytes.value // 8 + GUARD,), 0x5A5A5A5A5A5A, dtype=torch.int64, device=DEV)
    n = Q * k
    dist = torch.full((n + GUARD,), FILL_F, dtype=torch.float32, device=DEV)
    rows = torch.full((n + GUARD,), FILL_I, dtype=torch.int32, device=DEV)
    cert = torch.full((Q + GUARD,), FILL_I, dtype=torch.int32, device=DEV)
    keys = torch.full((Q * R + GUARD,), FILL_I, dtype=torch.int64, device=DEV) if want_keys else None
    rng = torch.zeros(2 + GUARD, dtype=torch.int32, device=DEV) if want_range else None
    t = [_dev(q, np.float32), _dev(g, np.float32), _dev(qq["codes"], np.int8), _dev(qq["scale"], np.float32), _dev(gq["codes"], np.int8),
         _dev(gq["scale"], np.float32), _dev(qq["rho"], np.float32), _dev(qq["norm"], np.float32), _dev(skip, np.int32)]
    rc = lib.fn_qgallery_search(_ptr(t[0]), Q, _ptr(t[1]), G, _ptr(t[2]), _ptr(t[3]), _ptr(t[4]), _ptr(t[5]), _ptr(t[6]), _ptr(t[7]),
                                float(gq["rho"].max()), float(gq["norm"].max()), E, k, R, metric, _ptr(t[8]), slab_rows, _ptr(ws), _ptr(dist),
                                _ptr(rows), _ptr(cert), _ptr(keys), _ptr(rng), _stream())
    torch.cuda.synchronize()
    out = {"rc": rc, "dist": dist.cpu().numpy(), "rows": rows.cpu().numpy(), "certified": cert.cpu().numpy()}
    if rc != 0:
        return out
    assert (out["dist"][n:] == FILL_F).all() and (out["rows"][n:] == FILL_I).all() and (out["certified"][Q:] == FILL_I).all()
    assert (ws[nbytes.value // 8:] == 0x5A5A5A5A5A5A).all()
    out["dist"], out["rows"] = out["dist"][:n].reshape(Q, k), out["rows"][:n].reshape(Q, k)
    out["certified"] = out["certified"][:Q]
    assert np.isin(out["certified"], (0, 1)).all()
    if keys is not None:
        words = keys.cpu().numpy()
        assert (words[Q * R:] == FILL_I).all()
        out["keys"] = words[:Q * R].view(np.uint64).reshape(Q, R)
    if rng is not None:
        words = rng.cpu().tolist()
        assert words[2:] == [0] * GUARD
        out["range"] = (_decode_ord(words[0]), _decode_ord(words[1]))
    return out


def check(got, ref, metric=0):
    """Everything fn_qgallery_search writes against the oracle's."""
    assert got["rc"] == 0
    if "keys" in got:
        assert np.array_equal(got["keys"], ref["keys"])
    assert np.array_equal(got["rows"], ref["rows"])
    assert np.array_equal(got["certified"].astype(bool), ref["certified"])
    if metric == 0:
        assert np.array_equal(got["dist"].view(np.uint32), ref["dist"].view(np.uint32))          # bit for bit
    else:
        ok = ref["rows"] >= 0
        assert np.isposinf(got["dist"][~ok]).all()
        err = np.abs(got["dist"][ok].astype(np.float64) - ref["dist"][ok])
        assert (err <= 8 * 2.0 ** -24 * np.abs(ref["dist"][ok])).all(), err.max()
    if "range" in got and ref["range"] is not None:
        assert got["range"] == ref["range"]


# ---- fn_quantize_rows ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 65])
@pytest.mark.parametrize("E", [4, 40, 72, 512])
def test_quantize_rows_bits(N, E):
    """E = 4 leaves 60 padded bytes per row; N = 65 is more than one workgroup of four waves and a ragged last one."""
    x = io.unit_rows(N, E, 10 * E + N)
    if N > 3:
        x[1] = 0                                               # a zero row: codes and scale 0
        x[2, E - 1] = -2 * np.abs(x[2]).max()                  # the maximum is a negative entry
        x[3] *= np.float32(1.001)
    same_quantisation(gpu_quantize(x), qo.quantize(x))


def test_quantize_rows_round_half_to_even():
    """m = 127 2^-8 and x_e = (j + 1/2) 2^-8: x 127 / m lands on exact halves."""
    j = np.arange(0, 60)
    row = np.concatenate([[127.0], j + 0.5, -(j + 0.5), np.zeros(3)]) * 2.0 ** -8          # E = 124
    x = np.stack([row, -row, row[::-1]]).astype(np.float32)
    ref = qo.quantize(x)
    even = np.where(j % 2 == 0, j, j + 1)
    assert np.array_equal(ref["codes"][0, 1:61].astype(np.int64), even)
    same_quantisation(gpu_quantize(x), ref)


# ---- the shortlist and the final results --------------------------------------------------------------------------------------
SHAPES = [(1, 1, 4, 1, 1), (1, 63, 40, 2, 5), (16, 150, 36, 3, 7), (17, 65, 72, 64, 64), (65, 300, 512, 5, 10),
          (3, 5, 8, 7, 9)]                                     # Q, G, E, k, R; the last: k and R beyond G


@functools.lru_cache(maxsize=None)
def shape_case(Q, G, E, k, R):
    q, g = io.unit_rows(Q, E, 1000 + Q), io.unit_rows(G, E, 2000 + G)
    s = io.chain_similarities(q, g)
    return q, g, {m: qo.search(q, g, k, R, metric=m, s=s) for m in (0, 1)}


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("Q,G,E,k,R", SHAPES)
def test_shapes(Q, G, E, k, R, metric):
    """Shortlist keys, rows, distances, certificates and range: ragged query and gallery tiles, a ragged code chunk (Ep = 64 of
    128), Q <= 16 (the waves split the column tiles) and R > G with its all-ones tail."""
    q, g, ref = shape_case(Q, G, E, k, R)
    got = gpu_qsearch(q, g, k, R, metric=metric)
    check(got, ref[metric], metric)
    if R > G:
        assert (got["keys"][:, G:] == qo.NONE).all() and got["certified"].all()
    if k > G:
        assert (got["rows"][:, G:] == -1).all() and np.isposinf(got["dist"][:, G:]).all()


def test_slabs_give_the_same_result():
    """slab_rows = 64 at G = 300: five slabs through the merge; the library's own choice returns identical arrays."""
    q, g, ref = shape_case(65, 300, 512, 5, 10)
    many, one = gpu_qsearch(q, g, 5, 10, slab_rows=64), gpu_qsearch(q, g, 5, 10)
    check(many, ref[0])
    for name in ("keys", "rows", "certified"):
        assert np.array_equal(many[name], one[name])
    assert np.array_equal(many["dist"].view(np.uint32), one["dist"].view(np.uint32))
    q, g, ref = shape_case(16, 150, 36, 3, 7)                  # the split arrangement with two slabs
    check(gpu_qsearch(q, g, 3, 7, slab_rows=128), ref[0])


@pytest.mark.parametrize("Q,G", [(5, 1100), (17, 4165)])
def test_many_lists_are_merged_in_groups(Q, G):
    """More than 64 partial lists per query (18 slabs of four lists; 66 slabs of one): groups of 32 are cut to R keys by a wave
    each before the re-rank, the last group ragged.  The same arrays as with the library's own slabs."""
    q, g = io.unit_rows(Q, 8, 3000 + Q), io.unit_rows(G, 8, 4000 + G)
    ref = qo.search(q, g, 3, 9)
    many, one = gpu_qsearch(q, g, 3, 9, slab_rows=64), gpu_qsearch(q, g, 3, 9)
    check(many, ref)
    check(one, ref)


def test_skip_and_optional_outputs():
    pool = io.unit_rows(70, 24, 21)
    skip = np.arange(70, dtype=np.int32)
    ref = qo.search(pool, pool, 4, 12, skip=skip)
    got = gpu_qsearch(pool, pool, 4, 12, skip=skip)
    check(got, ref)
    assert ((got["keys"] & np.uint64(0xFFFFFFFF)) != skip[:, None].astype(np.uint64)).all() and (got["rows"] != skip[:, None]).all()
    plain = gpu_qsearch(pool, pool, 4, 12, skip=np.full(70, -1, np.int32))
    check(plain, qo.search(pool, pool, 4, 12, s=ref["s"]))
    assert (plain["rows"][:, 0] == skip).all()                 # without skip every row finds itself first
    bare = gpu_qsearch(pool, pool, 4, 12, skip=skip, want_keys=False, want_range=False)      # both optional outputs NULL
    assert bare["rc"] == 0 and np.array_equal(bare["rows"], got["rows"])


@pytest.mark.parametrize("E", [64, 128])
def test_integer_codes_pair_equal_k(E):
    """Rows whose codes are distinct small integers: s^ = idot 2^-26 exactly, and the query and gallery tables differ, so a wrong
    k pairing inside the MFMA operands or a swapped row / column changes the keys."""
    q, cq = qo.small_integer_codes(20, E, 1)
    g, cg = qo.small_integer_codes(70, E, 2)
    ref = qo.search(q, g, 3, 16)
    assert np.array_equal(ref["est"].astype(np.float64), (cq @ cg.T) * 2.0 ** -26)
    assert len(np.unique(ref["keys"] >> np.uint64(32))) > 100                  # the distances tell the pairs apart
    check(gpu_qsearch(q, g, 3, 16), ref)


def test_argument_rules():
    lib = _lib.load()
    q, g = io.unit_rows(2, 8, 1), io.unit_rows(3, 8, 2)
    assert gpu_qsearch(q, g, 1, 2)["rc"] == 0
    for k, R in ((0, 1), (65, 64), (2, 1), (1, 65)):
        got = gpu_qsearch_refused(q, g, k, R)
        assert got["rc"] == -1 and (got["dist"] == FILL_F).all() and (got["rows"] == FILL_I).all()
    assert "shortlist must be in [k, 64]" in lib.fn_last_error().decode()
    for E in (0, 6, 516):
        assert gpu_qsearch_refused(q, g, 1, 2, E=E)["rc"] == -1 and "multiple of 4" in lib.fn_last_error().decode()
    assert gpu_qsearch_refused(q, g, 1, 2, metric=2)["rc"] == -1 and lib.fn_last_error().decode() == "Undefined similarity metric 2"


def gpu_qsearch_refused(q, g, k, R, E=None, metric=0):
    """A call the library must refuse: the workspace query is left out, the outputs stay as they were."""
    lib = _lib.load()
    Q, G, E = q.shape[0], g.shape[0], q.shape[1] if E is None else E
    qq, gq = qo.quantize(q), qo.quantize(g)
    ws = torch.zeros(1024, dtype=torch.int64, device=DEV)
    dist = torch.full((256,), FILL_F, dtype=torch.float32, device=DEV)
    rows = torch.full((256,), FILL_I, dtype=torch.int32, device=DEV)
    cert = torch.full((16,), FILL_I, dtype=torch.int32, device=DEV)
    t = [_dev(q, np.float32), _dev(g, np.float32), _dev(qq["codes"], np.int8), _dev(qq["scale"], np.float32), _dev(gq["codes"], np.int8),
         _dev(gq["scale"], np.float32), _dev(qq["rho"], np.float32), _dev(qq["norm"], np.float32)]
    rc = lib.fn_qgallery_search(_ptr(t[0]), Q, _ptr(t[1]), G, *map(_ptr, t[2:]), 1.0, 1.0, E, k, R, metric, None, 0, _ptr(ws), _ptr(dist), _ptr(rows),
                                _ptr(cert), None, None, _stream())
    torch.cuda.synchronize()
    return {"rc": rc, "dist": dist.cpu().numpy(), "rows": rows.cpu().numpy()}


# ---- the public path: exact on every input ------------------------------------------------------------------------------------
def same_as_gallery(qg, gal, q, k, **kw):
    got, want = qg.search(q, k=k, **kw), gal.search(q, k=k, **{n: v for n, v in kw.items() if n != "shortlist"})
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32))
    return want


@pytest.mark.parametrize("metric", [0, 1])
def test_exact_search_is_gallery_search(metric):
    from facenet_amd.recognize import Gallery, QuantizedGallery
    q, g = io.unit_rows(20, 128, 1), io.unit_rows(500, 128, 2)                  # random rows: every query certified
    gal = Gallery(g, metric=metric, device=DEV)
    qg = gal.quantize()
    assert isinstance(qg, QuantizedGallery) and qg.codes.shape == (500, 128) and qg.codes.dtype == torch.int8
    same_quantisation({"codes": qg.codes.cpu().numpy(), "scale": qg.scale.cpu().numpy(), "rho": qg.rho.cpu().numpy(),
                       "norm": qg.norm.cpu().numpy()}, qo.quantize(g))
    assert (qg.rho_max, qg.norm_max) == (float(qg.rho.max()), float(qg.norm.max()))
    same_as_gallery(qg, gal, q, 5)
    assert qg.last_fallbacks == 0
    dist, rows, certified = qg.search_certified(q, k=5)
    assert certified.dtype == bool and certified.all()
    dev_out = qg.search(torch.from_numpy(q).to(DEV), k=5, exact=False, atol=None)
    assert dev_out[0].is_cuda and np.array_equal(dev_out[1].cpu().numpy(), rows)

    g = qo.near_duplicates(3, 40, 128, 5, spread=0.011)                           # classes of 40 near-duplicates at k = 1, shortlist 16
    q = g[::4].copy()
    gal = Gallery(g, metric=metric, device=DEV)
    qg = gal.quantize(16)
    same_as_gallery(qg, gal, q, 1)
    ref = qo.search(q, g, 1, 16)
    assert qg.last_fallbacks == int((~ref["certified"]).sum()) > 0
    assert np.array_equal(qg.search_certified(q, k=1)[2], ref["certified"])
    skip = (np.arange(len(q)) * 4).astype(np.int32)
    same_as_gallery(qg, gal, q, 1, skip=skip)                                     # the fallback takes its queries' skip along
    assert qg.last_fallbacks > 0


def test_exact_search_with_ties_across_the_shortlist_boundary():
    """The +-1/8 pool quantises without error, so equal rows tie in s^ as they do in s: 24 copies of one row straddle a shortlist
    of 16, and the lower rows must win."""
    from facenet_amd.recognize import Gallery
    pool = io.tie_pool(300, 3)
    q, g = pool[:5].copy(), pool[5:].copy()
    copies = np.arange(3, 291, 12)                                                # 24 rows, across the 64-row tiles
    g[copies] = q[0]
    g[200], g[7] = q[1], q[1]
    gal = Gallery(g, device=DEV)
    qg = gal.quantize(16)
    want = same_as_gallery(qg, gal, q, 3)
    assert want[1][0].tolist() == copies[:3].tolist() and want[1][1, :2].tolist() == [7, 200] and qg.last_fallbacks > 0
    keys = gpu_qsearch(q, g, 3, 16)["keys"]
    assert (keys[0] & np.uint64(0xFFFFFFFF)).tolist() == copies[:16].tolist()     # the shortlist itself cuts the tie by row
    want = same_as_gallery(qg, gal, q, 3, slab_rows=64)
    same_as_gallery(gal.quantize(64), gal, q, 20)


def test_exact_search_on_the_adversarial_order():
    from facenet_amd.recognize import Gallery
    q, g = io.adversarial_order(1024, 32, 11)
    gal = Gallery(g, device=DEV)
    for k, R in ((1, 16), (5, 64), (64, 64)):
        qg = gal.quantize(R)
        want = same_as_gallery(qg, gal, q, k)
        same_as_gallery(qg, gal, q, k, slab_rows=256)
    assert want[1][0, 0] == 1023


# ---- end to end ---------------------------------------------------------------------------------------------------------------
def test_leave_one_out_and_identify():
    from facenet_amd.recognize import Gallery
    g = qo.near_duplicates(10, 7, 32, 9, spread=0.05)
    labels = np.repeat(np.arange(10), 7)
    names = {int(c): f"person{c}" for c in range(10)}
    gal = Gallery(g, labels=labels, names=names, device=DEV)
    qg = gal.quantize(32)
    for a, b in zip(qg.leave_one_out(4), gal.leave_one_out(4)):
        assert a.is_cuda and torch.equal(a, b)
    for a, b in zip(qg.leave_one_out(4, shortlist=8, exact=False), gal.leave_one_out(4)):
        assert a.shape == b.shape
    q = io.unit_rows(6, 32, 4)
    q[:3] = g[[3, 30, 66]]
    closed = gal.identify(q)
    assert qg.identify(q) == closed and qg.identify(q, k=3, shortlist=8) == closed and [c[3] for c in closed[:3]] == [3, 30, 66]
    thr = 0.5
    want = gal.identify(q, threshold=thr)
    assert any(w[0] == -1 for w in want) and any(w[0] >= 0 for w in want) and qg.identify(q, threshold=thr, shortlist=16) == want
    with pytest.raises(ValueError, match="embeddings must be normalized to 1, range"):
        qg.search(q * np.float32(1.5), k=2)


def test_face_pipeline_identifies_through_a_quantised_gallery(tmp_path):
    """FacePipeline.identify hands the device embeddings to whatever gallery it is given: a QuantizedGallery answers as the
    Gallery it was built from.  The network is a stand-in (pixel statistics of the crop, normalised)."""
    from facenet_amd.detectors.face_detector import FaceDetector
    from facenet_amd.recognize import FacePipeline, Gallery
    from oracle import mtcnn_oracle as mo
    np.savez(tmp_path / "w.npz", **mo.random_weights(0, face_bias=(0.5, 1.0, 1.0)))      # the synthetic detector of tests/test_gpu_mtcnn.py

    def evaluate_device(batch):
        x = batch.float().reshape(batch.shape[0], 16, -1).mean(dim=2) - 127.5
        return torch.nn.functional.normalize(x, dim=1)

    rng = np.random.default_rng(1)
    base = rng.integers(0, 256, (15, 20, 3), dtype=np.uint8)
    frame = np.clip(np.kron(base, np.ones((8, 8, 1), np.uint8)).astype(np.int32) + rng.integers(-12, 13, (120, 160, 3)), 0, 255).astype(np.uint8)
    pipeline = FacePipeline(FaceDetector(detector="pypimtcnn", weights_file=str(tmp_path / "w.npz")), SimpleNamespace(evaluate_device=evaluate_device),
                            SimpleNamespace(size=160, margin=0.25))
    boxes, crops = pipeline.crops(frame)
    assert len(boxes) > 1
    emb = pipeline.embed_device(crops)
    known = torch.cat([emb, torch.from_numpy(io.unit_rows(30, 16, 3)).to(DEV)])
    gal = Gallery(known, labels=np.arange(len(known)) % 5, device=DEV)
    want = pipeline.identify(frame, gal)
    got = pipeline.identify(frame, gal.quantize(), shortlist=8)
    assert [b.info() for b, _ in got] == [b.info() for b, _ in want] and [w for _, w in got] == [w for _, w in want]
    assert all(0 <= w[3] < len(known) for _, w in got)


def test_app_quantises_the_gallery_when_asked(tmp_path):
    """apps/identify.py: with identify.quantized the gallery of the options is a QuantizedGallery with the shortlist asked for,
    and its answers are the plain gallery's; without it, a Gallery as before."""
    from facenet_amd.apps import identify as app
    from facenet_amd.recognize import QuantizedGallery
    rows = io.unit_rows(200, 64, 5)
    np.savez(tmp_path / "g.npz", embeddings=rows, labels=np.arange(200) % 12)
    base = {"dataset": {"path": str(tmp_path / "photos")}, "gallery": {"path": str(tmp_path / "g.npz")}}
    plain, thr = app.load_gallery(app.load_options(overrides=dict(base, identify={"threshold": 0.5})))
    assert type(plain).__name__ == "Gallery" and thr == np.float32(0.5)
    qg, thr = app.load_gallery(app.load_options(overrides=dict(base, identify={"threshold": 0.5, "quantized": True, "shortlist": 16, "k": 3})))
    assert isinstance(qg, QuantizedGallery) and qg.shortlist == 16 and thr == np.float32(0.5)
    assert app.load_gallery(app.load_options(overrides=dict(base, identify={"quantized": True})))[0].shortlist == 64
    q = torch.from_numpy(rows[:9]).to(DEV)
    for a, b in zip(qg.search(q, k=3), plain.search(q, k=3)):
        assert torch.equal(a, b)
