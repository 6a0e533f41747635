"""fn_gallery_search / Gallery on the MI355X against the NumPy oracle (tests/identify_oracle.py): rows and metric-0 distances bit
for bit, metric-1 distances within the 4-ulp acosf rule of tests/test_gpu_loss_edges.py.  Output buffers are over-allocated and
pre-filled, so a write past [Q, k] is seen."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from facenet_amd import _lib
from facenet_amd.statistics import _decode_ord, cmc
from tests import identify_oracle as io

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 7                      # extra words behind every output buffer
FILL_F, FILL_I = -77.0, -77


def _dev(a, dtype):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def _ptr(t):
    return None if t is None else t.data_ptr()


def gpu_search(q, g, k, metric=0, skip=None, labels=None, slab_rows=0, want_labels=None, want_range=True):
    """One fn_gallery_search call -> dict(rc, dist, rows, labels, range (lo, hi) floats); the guard words are checked here."""
    lib = _lib.load()
    Q, G, E = q.shape[0], g.shape[0], q.shape[1]
    nbytes = C.c_longlong(-1)
    rc = lib.fn_gallery_search_workspace(Q, G, k, slab_rows, C.byref(nbytes))
    assert rc == 0 and nbytes.value >= Q * k * 8 and nbytes.value % (Q * k * 8) == 0
    ws = torch.full((nbytes.value // 8 + GUARD,), 0x5A5A5A5A5A5A, dtype=torch.int64, device=DEV)
    n = Q * k
    dist = torch.full((n + GUARD,), FILL_F, dtype=torch.float32, device=DEV)
    rows = torch.full((n + GUARD,), FILL_I, dtype=torch.int32, device=DEV)
    want_labels = labels is not None if want_labels is None else want_labels
    lab = torch.full((n + GUARD,), FILL_I, dtype=torch.int32, device=DEV) if want_labels else None
    rng = torch.zeros(2 + GUARD, dtype=torch.int32, device=DEV) if want_range else None
    qd, gd, sd, ld = _dev(q, np.float32), _dev(g, np.float32), _dev(skip, np.int32), _dev(labels, np.int32)
    rc = lib.fn_gallery_search(_ptr(qd), Q, _ptr(gd), G, E, k, metric, _ptr(sd), _ptr(ld), slab_rows, _ptr(ws), _ptr(dist), _ptr(rows),
                               _ptr(lab), _ptr(rng), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = {"rc": rc, "dist": dist.cpu().numpy(), "rows": rows.cpu().numpy(), "labels": None if lab is None else lab.cpu().numpy()}
    if rc != 0:
        return out
    assert (out["dist"][n:] == FILL_F).all() and (out["rows"][n:] == FILL_I).all()
    assert (ws[nbytes.value // 8:] == 0x5A5A5A5A5A5A).all()
    out["dist"], out["rows"] = out["dist"][:n].reshape(Q, k), out["rows"][:n].reshape(Q, k)
    if lab is not None:
        assert (out["labels"][n:] == FILL_I).all()
        out["labels"] = out["labels"][:n].reshape(Q, k)
    if rng is not None:
        words = rng.cpu().tolist()
        assert words[2:] == [0] * GUARD
        out["range"] = (_decode_ord(words[0]), _decode_ord(words[1]))
    return out


def check(got, ref, metric=0):
    assert got["rc"] == 0
    assert np.array_equal(got["rows"], ref["rows"])
    if metric == 0:
        assert np.array_equal(got["dist"].view(np.uint32), ref["dist"].view(np.uint32))          # bit for bit
    else:
        ok = ref["rows"] >= 0
        assert np.isposinf(got["dist"][~ok]).all()
        err = np.abs(got["dist"][ok].astype(np.float64) - ref["dist"][ok])
        assert (err <= 8 * 2.0 ** -24 * np.abs(ref["dist"][ok])).all(), err.max()
    if "range" in got:
        assert got["range"] == (float(ref["s"].min()), float(ref["s"].max()))


SHAPES = [(1, 1, 4, 1), (1, 63, 40, 5), (17, 65, 72, 64), (65, 300, 512, 10), (64, 129, 128, 1)]


@functools.lru_cache(maxsize=None)
def shape_case(Q, G, E, k):
    q, g = io.unit_rows(Q, E, 1000 + Q), io.unit_rows(G, E, 2000 + G)
    s = io.chain_similarities(q, g)
    return q, g, {m: io.search(q, g, k, metric=m, s=s) for m in (0, 1)}


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("Q,G,E,k", SHAPES)
def test_shapes(Q, G, E, k, metric):
    """Ragged query and gallery tiles, a ragged E chunk, k at its limit, and k > G with its -1 / inf tail."""
    q, g, ref = shape_case(Q, G, E, k)
    got = gpu_search(q, g, k, metric=metric)
    check(got, ref[metric], metric)
    if k > G:
        assert (got["rows"][:, G:] == -1).all() and np.isposinf(got["dist"][:, G:]).all()


def test_sixteen_queries_split_the_column_tiles():
    """Q <= 16: the four waves of a workgroup take one column tile each and keep lists of their own, merged as four slabs;
    Q = 16 is the last such shape (17 is in SHAPES).  Ragged gallery, a ragged E chunk, two slabs."""
    q, g = io.unit_rows(16, 36, 71), io.unit_rows(150, 36, 72)
    skip = np.arange(16, dtype=np.int32) * 9
    ref = io.search(q, g, 7, skip=skip)
    nbytes = C.c_longlong()
    assert _lib.load().fn_gallery_search_workspace(16, 150, 7, 128, C.byref(nbytes)) == 0 and nbytes.value == 2 * 4 * 16 * 7 * 8
    for slab_rows in (0, 128):
        check(gpu_search(q, g, 7, skip=skip, slab_rows=slab_rows), ref)


def test_slabs_and_merge():
    """slab_rows = 64 at G = 300: five slabs through the merge; the library's own choice returns identical arrays."""
    q, g, ref = shape_case(65, 300, 512, 10)
    nbytes = C.c_longlong()
    assert _lib.load().fn_gallery_search_workspace(65, 300, 10, 64, C.byref(nbytes)) == 0 and nbytes.value == 5 * 65 * 10 * 8
    assert _lib.load().fn_gallery_search_workspace(65, 300, 10, 1, C.byref(nbytes)) == 0 and nbytes.value == 5 * 65 * 10 * 8
    for metric in (0, 1):
        many, one = gpu_search(q, g, 10, metric=metric, slab_rows=64), gpu_search(q, g, 10, metric=metric)
        check(many, ref[metric], metric)
        assert np.array_equal(many["rows"], one["rows"]) and np.array_equal(many["dist"].view(np.uint32), one["dist"].view(np.uint32))


def test_exact_ties_go_to_the_lower_row():
    """The +-1/8 pool with duplicated rows across a slab boundary (63 | 64) and across the k-th position."""
    pool = io.tie_pool(200, 3)
    q = pool[:5].copy()
    g = pool[5:].copy()                       # 195 rows
    g[64] = g[63]                             # equal rows on both sides of the first slab boundary
    g[130] = g[20]
    g[63] = g[64] = q[0]                      # and both at distance 0 of query 0: ranks 1 and 2
    g[190] = q[1]
    g[7] = q[1]
    k = 3
    ref = io.search(q, g, k)
    assert ref["rows"][0, :2].tolist() == [63, 64] and ref["rows"][1, :2].tolist() == [7, 190]
    _, d0 = io.distances(ref["s"])
    kth = np.sort(d0, axis=1)[:, k - 1:k + 1]
    assert (kth[:, 0] == kth[:, 1]).any()      # some query has a tie across the k-th position
    results = [gpu_search(q, g, k, slab_rows=sr) for sr in (64, 128, 0)]
    for got in results:
        check(got, ref)
    ref1 = io.search(q, g, 1, s=ref["s"])
    check(gpu_search(q, g, 1, slab_rows=64), ref1)      # k-th position between the two duplicates


def test_far_candidates_never_lose_to_padding():
    """Every real row is at d0 > 2 of every query; a zero-padded column (s = 0, d0 = 2) would win if it could be selected."""
    q = io.unit_rows(3, 16, 8)
    noise = io.unit_rows(70, 16, 9).astype(np.float64)
    g = -q[0].astype(np.float64)[None, :] * 3 + noise
    g = (g / np.linalg.norm(g, axis=1, keepdims=True)).astype(np.float32)
    q = np.repeat(q[:1], 3, axis=0)
    ref = io.search(q, g, 10)
    assert (ref["dist"] > 2).all()
    for slab_rows in (0, 64):
        got = gpu_search(q, g, 10, slab_rows=slab_rows)
        check(got, ref)
        assert got["rows"].max() < 70 and got["rows"].min() >= 0
    few = gpu_search(q, g[:5], 10)             # k > G: the tail is -1 / inf, not a padding column at d0 = 2
    check(few, io.search(q, g[:5], 10))


def test_adversarial_order_prunes_every_tile():
    q, g = io.adversarial_order(1024, 32, 11)
    for k in (1, 5, 64):
        ref = io.search(q, g, k)
        check(gpu_search(q, g, k), ref)
        check(gpu_search(q, g, k, slab_rows=256), ref)
    assert ref["rows"][0, 0] == 1023


def test_skip_and_leave_one_out():
    from facenet_amd.recognize import Gallery
    pool = io.unit_rows(70, 24, 21)
    skip = np.arange(70, dtype=np.int32)
    ref = io.search(pool, pool, 4, skip=skip)
    got = gpu_search(pool, pool, 4, skip=skip)
    check(got, ref)
    assert (got["rows"] != skip[:, None]).all()
    none = gpu_search(pool, pool, 4, skip=np.full(70, -1, np.int32))
    plain = gpu_search(pool, pool, 4)
    assert np.array_equal(none["rows"], plain["rows"]) and np.array_equal(none["dist"].view(np.uint32), plain["dist"].view(np.uint32))
    assert (plain["rows"][:, 0] == skip).all()                           # without skip every row finds itself first
    dist, rows = Gallery(pool, device=DEV).leave_one_out(4)
    assert torch.is_tensor(dist) and dist.is_cuda and rows.dtype == torch.int32
    assert np.array_equal(rows.cpu().numpy(), ref["rows"]) and np.array_equal(dist.cpu().numpy(), ref["dist"])


def test_labels_and_tail():
    q, g = io.unit_rows(5, 8, 31), io.unit_rows(6, 8, 32)
    labels = np.array([9, 4, 4, 7, 0, 2 ** 31 - 1], dtype=np.int32)
    got = gpu_search(q, g, 8, labels=labels)
    check(got, io.search(q, g, 8))
    assert np.array_equal(got["labels"][:, :6], labels[got["rows"][:, :6]]) and (got["labels"][:, 6:] == -1).all()
    assert gpu_search(q, g, 8, labels=labels, want_labels=False, want_range=False)["rc"] == 0       # both optional outputs NULL


def test_range_and_normalisation_error():
    from facenet_amd.recognize import Gallery
    q, g = io.unit_rows(4, 16, 41), io.unit_rows(90, 16, 42)
    g[5] = q[2]
    q[2] *= np.float32(1.5)
    got = gpu_search(q, g, 2)
    s = io.chain_similarities(q, g)
    assert got["range"] == (float(s.min()), float(s.max())) and got["range"][1] > 1 + 1e-5
    gal = Gallery(g, device=DEV)
    with pytest.raises(ValueError, match="embeddings must be normalized to 1, range") as e:
        gal.search(q, k=2)
    assert str(e.value) == "\nembeddings must be normalized to 1, range {} {}".format(float(s.min()), float(s.max()))
    gal.search(io.unit_rows(4, 16, 41), k=2)
    dist, rows = gal.search(q, k=2, atol=None)                           # the check left out: nothing is read back, nothing raised
    assert np.array_equal(rows, io.search(q, g, 2, s=s)["rows"])


def test_argument_rules():
    """Every rule of the C ABI is refused with a message and without a launch (the pre-filled outputs stay as they were)."""
    lib = _lib.load()
    q, g = io.unit_rows(2, 8, 1), io.unit_rows(3, 8, 2)

    def refused(got):
        assert got["rc"] == -1 and lib.fn_last_error().decode() != ""
        assert (got["dist"] == FILL_F).all() and (got["rows"] == FILL_I).all()
        return lib.fn_last_error().decode()

    nbytes = C.c_longlong()
    for bad in ((0, 3, 1), (2, 0, 1), (2, 3, 0), (2, 3, 65)):
        assert lib.fn_gallery_search_workspace(*bad, 0, C.byref(nbytes)) == -1 and lib.fn_last_error().decode() != ""
    assert lib.fn_gallery_search_workspace(2, 3, 1, -1, C.byref(nbytes)) == -1

    def call(Q=2, G=3, E=8, k=1, metric=0, qoff=0, goff=0, wsoff=0, slab_rows=0, labels=True, row_labels=True, null=()):
        qd = torch.zeros(64, dtype=torch.float32, device=DEV)
        gd = torch.zeros(64, dtype=torch.float32, device=DEV)
        ws = torch.zeros(1024, dtype=torch.int64, device=DEV)
        dist = torch.full((256,), FILL_F, dtype=torch.float32, device=DEV)
        rows = torch.full((256,), FILL_I, dtype=torch.int32, device=DEV)
        lab = torch.zeros(64, dtype=torch.int32, device=DEV)
        out = torch.zeros(256, dtype=torch.int32, device=DEV)
        ptr = {"queries": qd.data_ptr() + qoff, "gallery": gd.data_ptr() + goff, "workspace": ws.data_ptr() + wsoff,
               "dist": dist.data_ptr(), "rows": rows.data_ptr()}
        ptr.update({name: None for name in null})
        rc = lib.fn_gallery_search(ptr["queries"], Q, ptr["gallery"], G, E, k, metric, None, lab.data_ptr() if labels else None,
                                   slab_rows, ptr["workspace"], ptr["dist"], ptr["rows"], out.data_ptr() if row_labels else None, None,
                                   torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return {"rc": rc, "dist": dist.cpu().numpy(), "rows": rows.cpu().numpy()}

    assert call()["rc"] == 0
    for kw in (dict(Q=0), dict(G=0), dict(k=0), dict(k=65)):
        refused(call(**kw))
    for E in (0, 2, 6, 516):
        assert "multiple of 4" in refused(call(E=E))
    for metric in (-1, 2):
        assert refused(call(metric=metric)) == f"Undefined similarity metric {metric}"
    assert "16-byte aligned" in refused(call(qoff=4))
    assert "16-byte aligned" in refused(call(goff=8))
    assert "16-byte aligned" in refused(call(wsoff=8))
    assert "bad arguments" in refused(call(slab_rows=-1))
    for name in ("queries", "gallery", "workspace", "dist", "rows"):
        assert "bad arguments" in refused(call(null=(name,)))
    assert "row_labels needs labels" in refused(call(labels=False))
    assert call(labels=False, row_labels=False)["rc"] == 0


def test_agrees_with_the_validation_kernel():
    """A threshold placed exactly on one distance: the neighbours below it (k = G, all rows) are twice the pairs that
    fn_confidence_counts bins below the same threshold for the same rows (one class: every pair a < b is counted once)."""
    lib = _lib.load()
    n, E = 40, 32
    pool = io.unit_rows(n, E, 51)
    ref = io.search(pool, pool, n, skip=np.arange(n))
    thr = np.float32(ref["dist"][3, n // 2])                            # the distance of one pair, exactly
    got = gpu_search(pool, pool, n, skip=np.arange(n, dtype=np.int32))
    check(got, ref)
    assert (got["rows"][:, n - 1] == -1).all()
    below = int(np.count_nonzero(got["dist"] < thr))
    assert below % 2 == 0 and 0 < below < n * (n - 1)
    assert np.count_nonzero(got["dist"] == thr) >= 2                    # the pair itself, from both sides: strict < leaves it out
    emb, cls = _dev(pool, np.float32), _dev(np.array([0, n]), np.int32)
    t_dev = _dev(np.array([thr]), np.float32)
    out = torch.zeros(4, dtype=torch.float64, device=DEV)
    rng = torch.zeros(2, dtype=torch.int32, device=DEV)
    _lib.check(lib.fn_confidence_counts(emb.data_ptr(), cls.data_ptr(), 1, E, t_dev.data_ptr(), 1, 0, out.data_ptr(), rng.data_ptr(),
                                        torch.cuda.current_stream().cuda_stream))
    pairs = n * (n - 1) // 2
    tp, fn = (out.cpu().numpy()[[0, 3]] * pairs).tolist()               # one class: weight = pairs * 1
    assert round(tp) + round(fn) == pairs and abs(tp - round(tp)) < 1e-6
    assert 2 * round(tp) == below


def test_gallery_identify_and_cmc():
    from facenet_amd.faceclass import FaceToFaceNormalizedEmbeddingsClassifier
    from facenet_amd.recognize import Gallery
    g = io.unit_rows(30, 16, 61)
    labels = np.repeat(np.arange(10), 3)
    labels[27:] = [10, 11, 12]                                          # three classes of one image
    names = {int(c): f"person{c}" for c in np.unique(labels)}
    gal = Gallery(g, labels=labels, names=names, device=DEV)
    noise = io.unit_rows(6, 16, 62).astype(np.float64)
    q = g[[4, 9, 29, 0, 13, 20]].astype(np.float64) + noise * np.array([0.05, 0.05, 0.05, 0.8, 0.8, 0.05])[:, None]
    q = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
    ref = io.search(q, g, 3)
    d, r = ref["dist"][:, 0], ref["rows"][:, 0]
    assert r[[0, 1, 2, 5]].tolist() == [4, 9, 29, 20]

    dist, rows = gal.search(q, k=3)
    assert isinstance(dist, np.ndarray) and np.array_equal(dist, ref["dist"]) and np.array_equal(rows, ref["rows"])
    dist_t, rows_t = gal.search(torch.from_numpy(q).to(DEV), k=3)
    assert dist_t.is_cuda and rows_t.is_cuda and np.array_equal(dist_t.cpu().numpy(), dist) and np.array_equal(rows_t.cpu().numpy(), rows)

    closed = [(int(labels[i]), names[int(labels[i])], float(x), int(i)) for x, i in zip(d, r)]
    assert gal.identify(q) == closed and gal.identify(torch.from_numpy(q).to(DEV), k=3) == closed
    thr = d[0]                                                          # exactly one face's distance: strict <, so it is unknown
    want = [c if x < thr else (-1, None, c[2], c[3]) for c, x in zip(closed, d)]
    assert any(w[0] == -1 for w in want) and any(w[0] >= 0 for w in want)
    assert gal.identify(q, threshold=float(thr)) == want
    clf = FaceToFaceNormalizedEmbeddingsClassifier(device=DEV)
    clf.params[1] = float(thr)
    assert gal.identify(q, classifier=clf) == want
    with pytest.raises(ValueError, match="not both"):
        gal.identify(q, threshold=1.0, classifier=clf)
    with pytest.raises(ValueError, match="metric 0"):
        Gallery(g, metric=1, device=DEV).identify(q, classifier=clf)
    assert Gallery(g, device=DEV).identify(q[:1]) == [(4, None, float(d[0]), 4)]          # no labels: the row is the label

    _, loo = gal.leave_one_out(5)
    want_cmc = cmc(labels, io.search(g, g, 5, skip=np.arange(30))["rows"])
    got_cmc = cmc(labels, loo.cpu().numpy())
    assert got_cmc[1] == want_cmc[1] == 3 and np.array_equal(got_cmc[0], want_cmc[0]) and (np.diff(got_cmc[0]) >= 0).all()
