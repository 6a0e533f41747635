"""fn_mate_search / Gallery.mates / IdentificationCurve on the MI355X against the NumPy oracle (tests/opensearch_oracle.py): rows,
ranks and metric-0 distances bit for bit, metric-1 distances within the 4-ulp acosf rule of tests/test_gpu_identify.py.  Every
buffer, the workspace included, is over-allocated and pre-filled, so a write past its end is seen."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from facenet_amd import _lib
from facenet_amd import statistics as st
from facenet_amd.statistics import _decode_ord
from tests import identify_oracle as io
from tests import opensearch_oracle as oo

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 7                      # extra words behind every buffer
FILL_F, FILL_I, FILL_W = -77.0, -77, 0x5A5A5A5A5A5A


def _dev(a, dtype):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def _ptr(t):
    return None if t is None else t.data_ptr()


def gpu_mates(q, qlabels, g, glabels, metric=0, skip=None, slab_rows=0, want_rank=True, want_range=True):
    """One fn_mate_search call -> dict(rc, dist [Q, 2], rows [Q, 2], ranks [Q] or None, range (lo, hi), workspace int64 words); the
    guard words are checked here."""
    lib = _lib.load()
    Q, G, E = q.shape[0], g.shape[0], q.shape[1]
    nbytes = C.c_longlong(-1)
    assert lib.fn_mate_search_workspace(Q, G, slab_rows, C.byref(nbytes)) == 0 and nbytes.value >= Q * 28
    words = -(-nbytes.value // 8)
    ws = torch.full((words + GUARD,), FILL_W, dtype=torch.int64, device=DEV)
    dist = torch.full((2 * Q + GUARD,), FILL_F, dtype=torch.float32, device=DEV)
    rows = torch.full((2 * Q + GUARD,), FILL_I, dtype=torch.int32, device=DEV)
    rank = torch.full((Q + GUARD,), FILL_I, dtype=torch.int32, device=DEV) if want_rank else None
    rng = torch.zeros(2 + GUARD, dtype=torch.int32, device=DEV) if want_range else None
    qd, gd, sd = _dev(q, np.float32), _dev(g, np.float32), _dev(skip, np.int32)
    qld, gld = _dev(qlabels, np.int32), _dev(glabels, np.int32)
    rc = lib.fn_mate_search(_ptr(qd), Q, _ptr(qld), _ptr(gd), G, _ptr(gld), E, metric, _ptr(sd), slab_rows, _ptr(ws), _ptr(dist), _ptr(rows),
                            _ptr(rank), _ptr(rng), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0
    out = {"rc": rc, "dist": dist.cpu().numpy(), "rows": rows.cpu().numpy(), "ranks": None if rank is None else rank.cpu().numpy(),
           "workspace": ws.cpu().numpy(), "nbytes": nbytes.value}
    assert (out["dist"][2 * Q:] == FILL_F).all() and (out["rows"][2 * Q:] == FILL_I).all()
    assert (out["workspace"][words:] == FILL_W).all()
    if nbytes.value % 8:           # the last word's upper half lies behind the workspace
        assert int(out["workspace"][words - 1]) >> 32 == FILL_W >> 32
    out["dist"], out["rows"] = out["dist"][:2 * Q].reshape(Q, 2), out["rows"][:2 * Q].reshape(Q, 2)
    if rank is not None:
        assert (out["ranks"][Q:] == FILL_I).all()
        out["ranks"] = out["ranks"][:Q]
    if rng is not None:
        w = rng.cpu().tolist()
        assert w[2:] == [0] * GUARD
        out["range"] = (_decode_ord(w[0]), _decode_ord(w[1]))
    return out


def check(got, ref, metric=0):
    assert np.array_equal(got["rows"], ref["rows"])
    if got["ranks"] is not None:
        assert np.array_equal(got["ranks"], ref["ranks"])
    ok = ref["rows"] >= 0
    assert np.isposinf(got["dist"][~ok]).all()
    if metric == 0:
        assert np.array_equal(got["dist"].view(np.uint32), ref["dist"].view(np.uint32))          # bit for bit
    else:
        err = np.abs(got["dist"][ok].astype(np.float64) - ref["dist"][ok])
        assert (err <= 8 * 2.0 ** -24 * np.abs(ref["dist"][ok])).all(), err.max()
    if "range" in got:
        assert got["range"] == (float(ref["s"].min()), float(ref["s"].max()))


@functools.lru_cache(maxsize=None)
def ragged_case():
    """Q = 70 (two query tiles, the second with 6 rows: three waves not live), G = 300 (slab_rows = 64: five slabs, a partial last
    super-tile), E = 36 (two chunks, the second partial), 7 ragged classes with a class of one; queries of every class, of a label
    the gallery lacks (-1) and with skip rows."""
    q, g = io.unit_rows(70, 36, 1070), io.unit_rows(300, 36, 2300)
    glabels = oo.ragged_labels([90, 1, 47, 3, 70, 64, 25], 5)
    qlabels = np.random.default_rng(6).integers(-1, 7, 70)
    skip = np.random.default_rng(7).integers(-1, 300, 70)
    s = io.chain_similarities(q, g)
    return q, qlabels, g, glabels, skip, {m: oo.mates(q, qlabels, g, glabels, metric=m, skip=skip, s=s) for m in (0, 1)}


@pytest.mark.parametrize("metric", [0, 1])
def test_ragged_shape_and_slabs(metric):
    """The same result for every slab height: five slabs, three, one (0: the library's choice) and one of 320 rows."""
    q, ql, g, gl, skip, ref = ragged_case()
    assert set(np.unique(ql)) == set(range(-1, 7)) and (ref[0]["ranks"] > 64).any() and (ref[0]["ranks"] == -1).any()
    nbytes = C.c_longlong()
    for slab_rows, slabs in ((64, 5), (128, 3), (0, 1), (320, 1)):
        assert _lib.load().fn_mate_search_workspace(70, 300, slab_rows, C.byref(nbytes)) == 0 and nbytes.value == slabs * 70 * 20 + 70 * 8
        check(gpu_mates(q, ql, g, gl, metric=metric, skip=skip, slab_rows=slab_rows), ref[metric], metric)


@pytest.mark.parametrize("Q,G,E", [(5, 70, 4), (20, 130, 512), (1, 1, 8), (64, 129, 128)])
def test_embedding_lengths(Q, G, E):
    q, g = io.unit_rows(Q, E, 1000 + Q), io.unit_rows(G, E, 2000 + G)
    gl, ql = np.arange(G) % 3, np.arange(Q) % 4 - 1
    s = io.chain_similarities(q, g)
    for metric in (0, 1):
        check(gpu_mates(q, ql, g, gl, metric=metric), oo.mates(q, ql, g, gl, metric=metric, s=s), metric)


def test_exact_ties_go_to_the_lower_row():
    """The +-1/8 pool: a tied mate pair across the first slab boundary (63 | 64, also a super-tile boundary) and a tied impostor
    pair across a super-tile boundary inside a slab (127 | 128 at slab_rows = 256) and across a slab boundary at 128."""
    pool = io.tie_pool(330, 3)
    q, g = pool[:5].copy(), pool[5:].copy()                # 325 rows
    gl = np.arange(325) % 4
    ql = np.array([0, 1, 2, 3, 0])
    gl[63] = gl[64] = 0
    g[63] = g[64] = q[0]                                   # mates of query 0, both at distance 0
    gl[127] = gl[128] = 1
    g[127] = g[128] = q[0]                                 # impostors of query 0, both at distance 0: behind the mate, rank 0
    gl[191] = gl[192] = 3
    g[191] = g[192] = q[1]                                 # impostors of query 1 at distance 0, its mates elsewhere: rank >= 2
    gl[100], gl[200], gl[260] = 1, 0, 2
    g[100] = g[200] = g[260] = q[4]                        # query 4: an impostor at distance 0 below its mate's row and one above: rank 1
    ref = oo.mates(q, ql, g, gl)
    assert ref["rows"][0].tolist() == [63, 127] and ref["ranks"][0] == 0 and ref["rows"][1, 1] == 191 and ref["ranks"][1] >= 2
    assert ref["rows"][4].tolist() == [200, 100] and ref["ranks"][4] == 1
    _, d0 = io.distances(ref["s"])
    assert all(len(np.unique(row)) < len(row) for row in d0)
    for slab_rows in (64, 128, 256, 0):
        check(gpu_mates(q, ql, g, gl, slab_rows=slab_rows), ref)
    skipped = oo.mates(q, ql, g, gl, skip=[63, 191, -1, -1, -1], s=ref["s"])
    assert skipped["rows"][0].tolist() == [64, 127] and skipped["ranks"][0] == 0 and skipped["rows"][1, 1] == 192
    for slab_rows in (64, 0):
        check(gpu_mates(q, ql, g, gl, skip=[63, 191, -1, -1, -1], slab_rows=slab_rows), skipped)


def test_far_rows_never_lose_to_padding():
    """Every real row is at d0 > 2 of every query, and one at d0 = 2 exactly: a zero-padded column (s = 0, d0 = 2, a lower or
    higher "row") would win, or tie, if it could be selected."""
    q = io.unit_rows(1, 16, 8)
    noise = io.unit_rows(70, 16, 9).astype(np.float64)
    g = -q[0].astype(np.float64)[None, :] * 3 + noise
    g = (g / np.linalg.norm(g, axis=1, keepdims=True)).astype(np.float32)
    q = np.repeat(q, 3, axis=0)
    gl, ql = np.arange(70) % 2, np.array([0, 1, -1])
    ref = oo.mates(q, ql, g, gl)
    assert (ref["dist"][ref["rows"] >= 0] > 2).all()
    for slab_rows in (0, 64):
        got = gpu_mates(q, ql, g, gl, slab_rows=slab_rows)
        check(got, ref)
        assert got["rows"].max() < 70
    e = np.zeros((2, 8), np.float32)
    e[0, 0] = e[1, 1] = 1                                  # orthogonal: s = 0, d0 = 2 exactly, as against zero padding
    ref = oo.mates(e[:1], [0], e[1:], [0])
    assert ref["rows"].tolist() == [[0, -1]] and ref["dist"][0, 0] == 2.0
    check(gpu_mates(e[:1], [0], e[1:], [0]), ref)
    check(gpu_mates(e[:1], [1], e[1:], [0]), oo.mates(e[:1], [1], e[1:], [0]))


def test_missing_populations():
    """No mate (a class of one under leave-one-out, a label the gallery lacks, label -1), no impostor (a one-class gallery), and
    neither (G = 1 with its only row skipped): row -1, +inf, rank -1."""
    x = io.unit_rows(9, 8, 13)
    got = gpu_mates(x[:4], [0, 1, 5, -1], x[4:], [0, 0, 1, 0, 0], skip=[-1, 2, -1, -1])
    ref = oo.mates(x[:4], [0, 1, 5, -1], x[4:], [0, 0, 1, 0, 0], skip=[-1, 2, -1, -1])
    check(got, ref)
    assert got["rows"][1:, 0].tolist() == [-1, -1, -1] and got["ranks"].tolist()[1:] == [-1, -1, -1] and got["ranks"][0] >= 0
    assert np.isposinf(got["dist"][1:, 0]).all() and (got["rows"][:, 1] >= 0).all()
    one = gpu_mates(x[:4], [0, 0, -1, 0], x[4:], [0, 0, 0, 0, 0])                       # one class: impostors only for the absent probe
    check(one, oo.mates(x[:4], [0, 0, -1, 0], x[4:], [0, 0, 0, 0, 0]))
    assert one["rows"][:, 1].tolist()[:2] == [-1, -1] and one["rows"][2, 1] >= 0 and one["ranks"].tolist() == [0, 0, -1, 0]
    for metric in (0, 1):
        none = gpu_mates(x[:1], [0], x[4:5], [0], metric=metric, skip=[0])
        assert none["rows"].tolist() == [[-1, -1]] and np.isposinf(none["dist"]).all() and none["ranks"].tolist() == [-1]
        s = io.chain_similarities(x[:1], x[4:5])
        assert none["range"] == (float(s[0, 0]), float(s[0, 0]))                         # the skipped pair is still in the range


def test_self_join_against_the_full_ordering():
    """G = 60: leave_one_out(k = 64) shows the whole ordering; the mate, the impostor and the rank are read off it."""
    from facenet_amd.recognize import Gallery, MateSearch
    x, labels = io.unit_rows(60, 24, 21), oo.ragged_labels([20, 1, 17, 2, 20], 9) * 1000 + 7       # any non-negative int64 is a label
    ref = oo.leave_one_out(x, labels)
    check(gpu_mates(x, labels // 1000, x, labels // 1000, skip=np.arange(60)), ref)
    gal = Gallery(x, labels=labels, device=DEV)
    found = gal.leave_one_out_mates()
    assert isinstance(found, MateSearch) and all(t.is_cuda for t in found) and found.ranks.dtype == found.mate_rows.dtype == torch.int32
    device_found, found = found, MateSearch(*(t.cpu().numpy() for t in found))
    dist, rows = (t.cpu().numpy() for t in gal.leave_one_out(64))
    for i in range(60):
        order = rows[i][rows[i] >= 0]
        assert len(order) == 59
        same = labels[order] == labels[i]
        first = int(np.argmax(same)) if same.any() else -1
        assert int(found.ranks[i]) == first == ref["ranks"][i]
        assert int(found.mate_rows[i]) == (order[first] if first >= 0 else -1)
        assert int(found.impostor_rows[i]) == order[np.argmax(~same)]
        assert float(found.impostor_dist[i]) == dist[i][np.argmax(~same)]
        assert float(found.mate_dist[i]) == (dist[i][first] if first >= 0 else np.inf)
    assert (found.ranks == -1).sum() == 1 and (found.ranks > 0).any()
    # NumPy in, NumPy out; ranks=False gives the same rows and no ranks
    host = gal.mates(x, labels, skip=np.arange(60))
    assert all(isinstance(a, np.ndarray) for a in host) and np.array_equal(host.ranks, ref["ranks"])
    assert np.array_equal(np.stack([host.mate_rows, host.impostor_rows], axis=1), ref["rows"])
    assert np.array_equal(np.stack([host.mate_dist, host.impostor_dist], axis=1), ref["dist"])
    quick = gal.leave_one_out_mates(ranks=False)
    assert quick.ranks is None and all(torch.equal(a, b) for a, b in zip(quick[:4], device_found[:4]))
    probes = gal.mates(x[:5], [labels[0], -1, 123456, labels[3], labels[4]])             # no skip: a probe finds itself first
    assert probes.mate_rows.tolist() == [0, -1, -1, 3, 4] and probes.impostor_rows[1] == 1 and probes.ranks.tolist() == [0, -1, -1, 0, 0]


def test_rank_null_runs_one_walk():
    """rank == NULL: the same rows and distances, and the second walk's counts in the workspace stay as the caller left them."""
    q, ql, g, gl, skip, ref = ragged_case()
    both = gpu_mates(q, ql, g, gl, skip=skip, slab_rows=64)
    one = gpu_mates(q, ql, g, gl, skip=skip, slab_rows=64, want_rank=False)
    assert one["ranks"] is None
    check(one, ref[0])
    counts_at = (5 * 70 * 2 + 70) * 8                      # behind the partial keys and the mate keys
    counts = lambda got: got["workspace"].view(np.int32)[counts_at // 4: got["nbytes"] // 4].reshape(5, 70)
    assert set(np.unique(counts(one)).tolist()) <= {FILL_W & 0xFFFFFFFF, FILL_W >> 32}       # the fill pattern's two halves: untouched
    mated = ref[0]["ranks"] >= 0
    assert np.array_equal(counts(both).sum(axis=0)[mated], ref[0]["ranks"][mated]) and (counts(both) >= 0).all()


def test_range_and_normalisation_error():
    from facenet_amd.recognize import Gallery
    q, g = io.unit_rows(4, 16, 41), io.unit_rows(90, 16, 42)
    g[5] = q[2]
    q[2] *= np.float32(1.5)
    gl, ql = np.arange(90) % 5, np.array([0, 1, 2, 3])
    s = io.chain_similarities(q, g)
    got = gpu_mates(q, ql, g, gl, skip=[-1, -1, 5, -1])
    assert got["range"] == (float(s.min()), float(s.max())) and got["range"][1] > 1 + 1e-5      # the skipped pair holds the maximum
    assert gpu_mates(q, ql, g, gl, want_range=False, want_rank=False)["rc"] == 0                # both optional outputs NULL
    gal = Gallery(g, labels=gl, device=DEV)
    with pytest.raises(ValueError, match="embeddings must be normalized to 1, range") as e:
        gal.mates(q, ql)
    assert str(e.value) == "\nembeddings must be normalized to 1, range {} {}".format(float(s.min()), float(s.max()))
    gal.mates(io.unit_rows(4, 16, 41), ql)
    found = gal.mates(q, ql, atol=None)                                  # the check left out: nothing raised
    assert np.array_equal(found.impostor_rows, oo.mates(q, ql, g, gl, s=s)["rows"][:, 1])


def test_argument_rules():
    """Every rule of the C ABI is refused with a message and without a launch (the pre-filled outputs stay as they were)."""
    lib = _lib.load()

    def call(Q=2, G=3, E=8, metric=0, qoff=0, goff=0, wsoff=0, slab_rows=0, null=()):
        qd = torch.zeros(64, dtype=torch.float32, device=DEV)
        gd = torch.zeros(64, dtype=torch.float32, device=DEV)
        ws = torch.zeros(1024, dtype=torch.int64, device=DEV)
        dist = torch.full((256,), FILL_F, dtype=torch.float32, device=DEV)
        rows = torch.full((256,), FILL_I, dtype=torch.int32, device=DEV)
        rank = torch.full((256,), FILL_I, dtype=torch.int32, device=DEV)
        ql = torch.zeros(64, dtype=torch.int32, device=DEV)
        gl = torch.zeros(64, dtype=torch.int32, device=DEV)
        ptr = {"queries": qd.data_ptr() + qoff, "gallery": gd.data_ptr() + goff, "workspace": ws.data_ptr() + wsoff, "dist": dist.data_ptr(),
               "rows": rows.data_ptr(), "query_labels": ql.data_ptr(), "gallery_labels": gl.data_ptr(), "rank": rank.data_ptr()}
        ptr.update({name: None for name in null})
        rc = lib.fn_mate_search(ptr["queries"], Q, ptr["query_labels"], ptr["gallery"], G, ptr["gallery_labels"], E, metric, None, slab_rows,
                                ptr["workspace"], ptr["dist"], ptr["rows"], ptr["rank"], None, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return {"rc": rc, "dist": dist.cpu().numpy(), "rows": rows.cpu().numpy(), "rank": rank.cpu().numpy()}

    def refused(got):
        assert got["rc"] == -1 and lib.fn_last_error().decode() != ""
        assert (got["dist"] == FILL_F).all() and (got["rows"] == FILL_I).all() and (got["rank"] == FILL_I).all()
        return lib.fn_last_error().decode()

    ok = call()
    assert ok["rc"] == 0 and (ok["rows"][:4] != FILL_I).all() and (ok["rank"][:2] != FILL_I).all() and (ok["rank"][2:] == FILL_I).all()
    assert call(null=("rank",))["rc"] == 0
    for kw in (dict(Q=0), dict(G=0), dict(Q=-1)):
        assert "at least 1" in refused(call(**kw))
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
    for name in ("query_labels", "gallery_labels"):
        assert "query_labels and gallery_labels must be given" in refused(call(null=(name,)))


def test_agrees_with_the_radius_search_and_identify():
    """A threshold placed exactly on one returned distance: the probes whose nearest impostor is below it are the probes with an
    impostor row in `Gallery.within(eps = t)`, and dir_at(t) counts the probes that `identify(threshold = t)` names correctly."""
    from facenet_amd.recognize import Gallery
    g, gl = io.unit_rows(80, 16, 51), oo.ragged_labels([30, 20, 1, 29], 2)
    noise = io.unit_rows(40, 16, 52).astype(np.float64)
    q = g[:40].astype(np.float64) + 0.6 * noise
    q = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
    ql = gl[:40].copy()
    ql[:4] = -1
    gal = Gallery(g, labels=gl, device=DEV)
    found = gal.mates(q, ql)
    t = float(np.sort(found.impostor_dist)[17])                         # one probe's impostor distance exactly: strict < leaves it out
    offsets, rows, _ = gal.within(q, t)
    want_fp = sum(1 for i in range(40) if (gl[rows[offsets[i]:offsets[i + 1]]] != ql[i]).any())
    assert want_fp == int((found.impostor_dist < np.float32(t)).sum()) and 0 < want_fp <= 17
    curve = st.IdentificationCurve.from_search(found.mate_dist, found.impostor_dist, found.ranks, impostor_rows=found.impostor_rows)
    at = curve.dir_at(t)
    assert at["false_positives"] == want_fp and curve.nrof_mated == 36
    # identify names the nearest row: correct exactly when the nearest row is the mate (rank 0) and nearer than the threshold
    named = gal.identify(q, threshold=t)
    assert at["hits"] == sum(1 for (label, _, _, _), want in zip(named, ql) if want >= 0 and label == want) and 0 < at["hits"] <= 36
    tm = float(found.mate_dist[np.isfinite(found.mate_dist)][5])          # and on a mate's distance
    named = gal.identify(q, threshold=tm)
    assert curve.dir_at(tm)["hits"] == sum(1 for (label, _, _, _), want in zip(named, ql) if want >= 0 and label == want) < 36


def test_identification_curve_end_to_end():
    n, E = 200, 32
    labels = oo.ragged_labels([60, 1, 45, 2, 1, 50, 41], 8)
    centres = io.unit_rows(7, E, 81).astype(np.float64)
    x = centres[labels] + 2.0 * io.unit_rows(n, E, 82).astype(np.float64)
    x = (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
    s = io.chain_similarities(x, x)
    for metric in (0, 1):
        ref = oo.mates(x, labels, x, labels, metric=0, skip=np.arange(n), s=s)              # ranks, rows and the order: metric 0's
        curve = st.IdentificationCurve(x, labels, metric=metric, device=DEV)
        assert (curve.nrof_probes, curve.nrof_mated, curve.nrof_nonmated) == (n, n - 2, n)
        assert np.array_equal(curve.ranks, ref["ranks"]) and np.array_equal(curve.impostor_rows, ref["rows"][:, 1])
        assert np.array_equal(curve.mate_rows, ref["rows"][:, 0]) and (curve.ranks > 64).any()
        fpirs = [0.0, 0.01, 0.1, 0.5, 1.0]
        for rank in (1, 5):
            got = curve.fnir_at_fpir(fpirs, rank=rank)
            want = oo.fnir_at_fpir(curve.mate_dist, curve.impostor_dist, ref["ranks"], fpirs, rank=rank)
            assert [{k: g[k] for k in w} for g, w in zip(got, want)] == want
            if metric == 0:        # the distances are the oracle's bits, so the whole record is the oracle's
                assert want == oo.fnir_at_fpir(ref["dist"][:, 0], ref["dist"][:, 1], ref["ranks"], fpirs, rank=rank)
        assert got[1]["false_positives"] <= 2 and got[2]["hits"] <= got[3]["hits"] <= got[4]["hits"] == int(((ref["ranks"] >= 0) & (ref["ranks"] < 5)).sum())
        want_cmc, left_out = st.cmc(labels, io.search(x, x, 64, skip=np.arange(n), s=s)["rows"])
        assert left_out == 2 and np.array_equal(curve.cmc(64)[0], want_cmc) and curve.cmc(64)[1] == 2
        assert np.array_equal(curve.cmc(199)[0], oo.cmc(ref["ranks"], 199)[0]) and curve.cmc(199)[0][-1] == 1.0
        assert [m[:2] for m in curve.mislabelled()] == [m[:2] for m in oo.mislabelled(curve.mate_dist, curve.impostor_dist, ref["rows"][:, 1], ref["ranks"])]
    with pytest.raises(ValueError, match="embeddings must be normalized to 1"):
        st.IdentificationCurve(1.01 * np.concatenate([x, x[:1]]), np.concatenate([labels, labels[:1]]), device=DEV)


# ---- the app and the callback -------------------------------------------------------------------------------------------------------
class _PixelModel:
    """In place of the network: the first 64 pixel values of an image, centred and normalised.  The app's wiring is under test."""

    def __init__(self, config):
        self.config = config

    def evaluate(self, images):
        x = torch.as_tensor(images).cpu().reshape(len(images), -1)[:, :64].to(torch.float32) - 127.5
        return torch.nn.functional.normalize(x, dim=1)


def test_validate_app_appends_the_curve(tmp_path, monkeypatch):
    from PIL import Image
    import facenet_amd.api
    from facenet_amd.apps.validate import load_options, validate
    monkeypatch.setattr(facenet_amd.api, "FaceNet", _PixelModel)
    rng = np.random.default_rng(0)
    data = tmp_path / "faces"
    for c, n in enumerate((7, 8)):
        (data / f"id_{c:03d}").mkdir(parents=True)
        for i in range(n):
            Image.fromarray(rng.integers(0, 256, (160, 160, 3), dtype=np.uint8)).save(data / f"id_{c:03d}" / f"img_{i:03d}.png")
    texts, reports = [], []
    for k, extra in enumerate(({}, {"fpir_targets": [0.1, 0.5], "fpir_rank": 2})):
        overrides = {"batch_size": 8, "dataset": {"path": str(data)}, "model": {"path": None},
                     "validate": dict({"nrof_folds": 3}, **extra), "file": str(tmp_path / f"report{k}.txt")}
        lines = []
        reports.append(validate(load_options(overrides=overrides), log=lambda s: lines.append(str(s))))
        texts.append(((tmp_path / f"report{k}.txt").read_text(), lines))
    (plain, plain_log), (full, full_log) = texts
    assert reports[0].identification is None and reports[0].curve is None
    assert "IdentificationCurve" not in plain and not any("IdentificationCurve" in l for l in plain_log)
    curve = reports[1].identification
    block = 64 * "-" + "\n" + str(curve)
    assert isinstance(curve, st.IdentificationCurve) and full.count(block) == 1 and str(curve) in full_log and reports[1].curve is None
    assert "FNIR @ FPIR = 0.1 (rank 2)\n" in block and "FNIR @ FPIR = 0.5 (rank 2)\n" in block
    assert (curve.nrof_mated, curve.nrof_nonmated) == (15, 15)
    # without the block the file has the lines it has without the key (dates and times apart): the report of before this key existed
    strip = lambda t: [l for l in t.split("\n") if not l.startswith(("FaceToFaceValidation 20", "elapsed time: ", str(tmp_path)))]
    assert strip(full.replace(block, "")) == strip(plain)
    assert full.index(block) > full.index("FalseAlarmRate(FAR = 0.001)") and full.split("\n")[-2].startswith("elapsed time: ")


def test_validate_callback_appends_the_curve(tmp_path):
    from facenet_amd import callbacks
    from facenet_amd.config import Config
    x, labels = io.unit_rows(90, 16, 91), oo.ragged_labels([30, 25, 1, 34], 4)
    data = [(x[:50], labels[:50]), (x[50:], labels[50:])]                  # the "images" are the embeddings: the model is the identity

    class Model:
        path = tmp_path / "run"

        def __call__(self, images):
            return images

    class Report:
        dict = {}

        def __init__(self, *a):
            pass

        def __repr__(self):
            return "stub report\n"

        def write_report(self, file):
            with open(file, "at") as f:
                f.write(str(self))

    lines = []
    cb = callbacks.ValidateCallback(Model(), data, 1, 1, Config({"validate": {"metric": 1, "fpir_targets": [0.5, 0.01]}}),
                                    log=lambda s: lines.append(str(s)), statistic=Report)
    report = cb.on_epoch_end(0)
    curve = report.identification
    assert isinstance(curve, st.IdentificationCurve) and curve.metric == 1 and not hasattr(report, "curve")
    assert (tmp_path / "run" / "report.txt").read_text() == "stub report\n" + 64 * "-" + "\n" + str(curve) and str(curve) in lines
    by_hand = st.IdentificationCurve(x, labels, metric=1, device=DEV)
    assert by_hand.fnir_at_fpir([0.01, 0.5]) == curve.fnir_at_fpir([0.01, 0.5]) and str(curve).count("FNIR @ FPIR = ") == 2
    assert str(curve).index("FNIR @ FPIR = 0.01 ") < str(curve).index("FNIR @ FPIR = 0.5 ")
