"""fn_kmeans_update, fn_ivf_search, Gallery.kmeans and IVFGallery on the MI355X against the NumPy oracle (tests/ivf_oracle.py): rows,
metric-0 distances and centroids bit for bit, metric-1 distances within the 4-ulp acosf rule of tests/test_gpu_identify.py.  Every
buffer a call writes is over-allocated and pre-filled, so a write past its end is seen."""
import ctypes as C
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from facenet_amd import _lib
from facenet_amd.statistics import _decode_ord
from tests import identify_oracle as io
from tests import ivf_oracle as vo

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 7                      # extra words behind every output buffer
FILL_F, FILL_I, FILL_W = -77.0, -77, 0x5A5A5A5A5A5A


def _dev(a, dtype):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ---- fn_kmeans_update ----------------------------------------------------------------------------------------------------------
def gpu_kmeans_update(rows, assign, prev):
    """One fn_kmeans_update call -> (centroids float32 [L, E], kept int32 [L]); the guard words are checked here."""
    lib = _lib.load()
    (N, E), L = rows.shape, prev.shape[0]
    order, list_start = vo.lists_of(assign, L)
    out = torch.full((L * E + GUARD,), FILL_F, dtype=torch.float32, device=DEV)
    kept = torch.full((L + GUARD,), FILL_I, dtype=torch.int32, device=DEV)
    rd, od, sd, pd = _dev(rows, np.float32), _dev(order, np.int32), _dev(list_start, np.int32), _dev(prev, np.float32)
    rc = lib.fn_kmeans_update(_ptr(rd), N, E, _ptr(od), _ptr(sd), L, _ptr(pd), _ptr(out), _ptr(kept), _stream())
    torch.cuda.synchronize()
    assert rc == 0, lib.fn_last_error().decode()
    out, kept = out.cpu().numpy(), kept.cpu().numpy()
    assert (out[L * E:] == FILL_F).all() and (kept[L:] == FILL_I).all()
    return out[:L * E].reshape(L, E), kept[:L]


@pytest.mark.parametrize("E", [4, 64, 512])
def test_kmeans_update_bits(E):
    """Lists of 0, 1, 2 (an antipodal pair: n2 == 0), 63, 64, 65 and 105 rows, their members scattered over the table."""
    sizes = [0, 1, 2, 63, 64, 65, 105]
    N, L = sum(sizes), len(sizes)
    assert N == 300
    rows = io.unit_rows(N, E, 100 + E)
    assign = np.random.default_rng(E).permutation(np.repeat(np.arange(L), sizes))
    pair = np.nonzero(assign == 2)[0]
    rows[pair[1]] = -rows[pair[0]]
    prev = io.unit_rows(L, E, 200 + E)
    want, want_kept = vo.kmeans_update(rows, assign, prev)
    assert want_kept.tolist() == [1, 0, 1, 0, 0, 0, 0]
    got, kept = gpu_kmeans_update(rows, assign, prev)
    assert np.array_equal(kept, want_kept)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(got[[0, 2]].view(np.uint32), prev[[0, 2]].view(np.uint32))          # kept bit for bit
    again, kept2 = gpu_kmeans_update(rows, assign, prev)
    assert np.array_equal(again.view(np.uint32), got.view(np.uint32)) and np.array_equal(kept2, kept)


# ---- fn_ivf_search -------------------------------------------------------------------------------------------------------------
def gpu_ivf_search(q, g, assign, L, probes, k, metric=0, skip=None, want_range=True):
    """One fn_ivf_search call on the index of `assign` -> dict(rc, dist, rows, range); the guard words are checked here."""
    lib = _lib.load()
    (Q, E), G, nprobe = q.shape, g.shape[0], probes.shape[1]
    ids, list_start = vo.lists_of(assign, L)
    nbytes = C.c_longlong(-1)
    assert lib.fn_ivf_search_workspace(Q, L, nprobe, E, k, C.byref(nbytes)) == 0 and nbytes.value % 8 == 0
    ws = torch.full((nbytes.value // 8 + GUARD,), FILL_W, dtype=torch.int64, device=DEV)
    n = Q * k
    dist = torch.full((n + GUARD,), FILL_F, dtype=torch.float32, device=DEV)
    rows = torch.full((n + GUARD,), FILL_I, dtype=torch.int32, device=DEV)
    rng = torch.zeros(2 + GUARD, dtype=torch.int32, device=DEV) if want_range else None
    qd, ld, idd, lsd = _dev(q, np.float32), _dev(g[ids], np.float32), _dev(ids, np.int32), _dev(list_start, np.int32)
    pd, sd = _dev(probes, np.int32), _dev(skip, np.int32)
    rc = lib.fn_ivf_search(_ptr(qd), Q, _ptr(ld), _ptr(idd), G, _ptr(lsd), L, E, _ptr(pd), nprobe, k, metric, _ptr(sd), _ptr(ws), _ptr(dist),
                           _ptr(rows), _ptr(rng), _stream())
    torch.cuda.synchronize()
    assert rc == 0, lib.fn_last_error().decode()
    out = {"rc": rc, "dist": dist.cpu().numpy(), "rows": rows.cpu().numpy()}
    assert (out["dist"][n:] == FILL_F).all() and (out["rows"][n:] == FILL_I).all()
    assert (ws[nbytes.value // 8:] == FILL_W).all()
    out["dist"], out["rows"] = out["dist"][:n].reshape(Q, k), out["rows"][:n].reshape(Q, k)
    if rng is not None:
        words = rng.cpu().tolist()
        assert words[2:] == [0] * GUARD
        out["range"] = (_decode_ord(words[0]), _decode_ord(words[1]))
    return out


def check(got, ref, metric=0):
    assert np.array_equal(got["rows"], ref["rows"])
    if metric == 0:
        assert np.array_equal(got["dist"].view(np.uint32), ref["dist"].view(np.uint32))          # bit for bit
    else:
        ok = ref["rows"] >= 0
        assert np.isposinf(got["dist"][~ok]).all()
        err = np.abs(got["dist"][ok].astype(np.float64) - ref["dist"][ok])
        assert (err <= 8 * 2.0 ** -24 * np.abs(ref["dist"][ok])).all(), err.max()
    if "range" in got:
        if ref["range"] is None:
            assert got["range"][1] < got["range"][0]           # no pair evaluated: the initial words
        else:
            assert got["range"] == ref["range"]


G, L, E = 300, 8, 64
SIZES = [0, 1, 65, 129, 30, 30, 30, 15]       # list 0 is empty, list 1 holds one row


@functools.lru_cache(maxsize=None)
def constructed():
    """The gallery, the assignment (members scattered over the table), 70 queries, their chain values and their probes: three
    distinct lists per query with -1 entries; query 0 probes the one-row list and the empty one (a tail for every k > 1), query 5
    probes nothing, and every query's first probe is list 3, so that at Q = 70 two descriptors serve that list."""
    assert sum(SIZES) == G and len(SIZES) == L
    g, q = io.unit_rows(G, E, 1), io.unit_rows(70, E, 2)
    assign = np.random.default_rng(3).permutation(np.repeat(np.arange(L), SIZES))
    rng = np.random.default_rng(4)
    probes = np.stack([np.concatenate([[3], rng.permutation([0, 1, 2, 4, 5, 6, 7])[:2]]) for _ in range(70)]).astype(np.int32)
    probes[rng.random(70) < 0.3, 2] = -1
    probes[rng.random(70) < 0.2, 1] = -1
    probes[0] = [1, 0, -1]
    probes[5] = -1
    s = io.chain_similarities(q, g)
    return g, q, assign, probes, s


@pytest.mark.parametrize("Q", [1, 16, 17, 70])
def test_constructed_lists(Q):
    g, q, assign, probes, s = constructed()
    q, probes, s = q[:Q], probes[:Q], s[:Q]
    near = vo.ivf_search(q, g, assign, probes, 1, s=s)["rows"][:, 0]
    unprobed = np.array([np.nonzero(~np.isin(assign, probes[i]))[0][0] for i in range(Q)])
    skip = np.where(np.arange(Q) % 3 == 0, near, np.where(np.arange(Q) % 3 == 1, unprobed, -1)).astype(np.int32)
    for k in (1, 5, 64):
        for metric in (0, 1):
            for sk in (None, skip):
                ref = vo.ivf_search(q, g, assign, probes, k, metric=metric, skip=sk, s=s)
                check(gpu_ivf_search(q, g, assign, L, probes, k, metric=metric, skip=sk), ref, metric)
    assert ref["rows"][0, 0] == -1 and (vo.ivf_search(q, g, assign, probes, 5, s=s)["rows"][0, 1:] == -1).all()      # query 0: one row, skipped
    if Q > 5:
        assert (ref["rows"][5] == -1).all()
    hit = np.arange(Q) % 3 == 0
    assert (ref["rows"][hit] != skip[hit][:, None]).all()
    assert gpu_ivf_search(q, g, assign, L, probes, 5, want_range=False)["rc"] == 0          # the optional output NULL


def test_nothing_probed_at_all():
    g, q, assign, _, s = constructed()
    probes = np.full((3, 2), -1, np.int32)
    ref = vo.ivf_search(q[:3], g, assign, probes, 4, s=s[:3])
    assert ref["range"] is None and (ref["rows"] == -1).all()
    check(gpu_ivf_search(q[:3], g, assign, L, probes, 4), ref)
    one_list = np.zeros(G, dtype=np.int64)                     # L = 1: a single list is the whole gallery
    ref = io.search(q[:20], g, 6, s=s[:20])
    got = gpu_ivf_search(q[:20], g, one_list, 1, np.zeros((20, 1), np.int32), 6)
    assert np.array_equal(got["rows"], ref["rows"]) and np.array_equal(got["dist"].view(np.uint32), ref["dist"].view(np.uint32))


def test_exact_ties_go_to_the_lower_original_row():
    """The +-1/8 pool: equal rows in DIFFERENT lists, the lower original row stored behind the higher one, at ranks 1 | 2 and
    across the k-th position."""
    pool = io.tie_pool(G + 5, 3)
    q, g = pool[:5].copy(), pool[5:].copy()
    assign = constructed()[2].copy()
    late, early = np.nonzero(assign == 7)[0], np.nonzero(assign == 2)[0]
    a, b = int(late[late < early.max()][0]), int(early.max())            # a < b, a's list is stored last
    assert a < b and assign[a] == 7 and assign[b] == 2
    g[a] = g[b] = q[0]
    c, d = int(np.nonzero(assign == 3)[0][0]), int(np.nonzero(assign == 4)[0][-1])
    g[c] = g[d] = q[1]
    probes = np.tile(np.array([2, 7, 3, 4], np.int32), (5, 1))
    ref = vo.ivf_search(q, g, assign, probes, 3)
    assert ref["rows"][0, :2].tolist() == [a, b] and ref["rows"][1, :2].tolist() == sorted([c, d])
    _, d0 = io.distances(ref["s"])
    probed = np.isin(assign, probes[0])
    kth = np.sort(d0[:, probed], axis=1)[:, 2:4]
    assert (kth[:, 0] == kth[:, 1]).any()                      # some query has a tie across the k-th position
    check(gpu_ivf_search(q, g, assign, L, probes, 3), ref)
    ref1 = vo.ivf_search(q, g, assign, probes, 1, s=ref["s"])
    assert ref1["rows"][0, 0] == a
    check(gpu_ivf_search(q, g, assign, L, probes, 1), ref1)     # the k-th position between the two duplicates
    check(gpu_ivf_search(q, g, assign, L, probes[:, ::-1].copy(), 1), ref1)      # the order of the probes changes nothing


def test_adversarial_order_inside_one_list():
    """List 3's 129 rows, in the order the walk meets them, each nearer to query 0 than all before: the prune path runs every time."""
    g, _, assign, _, _ = constructed()
    g = g.copy()
    members = np.nonzero(assign == 3)[0]
    q, rows = io.adversarial_order(len(members), E, 11)
    g[members] = rows
    probes = np.array([[3, 6], [3, -1], [2, 3]], np.int32)
    for k in (1, 5, 64):
        ref = vo.ivf_search(q, g, assign, probes, k)
        check(gpu_ivf_search(q, g, assign, L, probes, k), ref)
    assert ref["rows"][0, 0] == members[-1]


def gpu_gallery_search(q, g, k, metric, skip):
    lib = _lib.load()
    Q, Gn = q.shape[0], g.shape[0]
    nbytes = C.c_longlong(-1)
    assert lib.fn_gallery_search_workspace(Q, Gn, k, 0, C.byref(nbytes)) == 0
    ws = torch.zeros(nbytes.value // 8 + 1, dtype=torch.int64, device=DEV)
    dist, rows = torch.empty((Q, k), dtype=torch.float32, device=DEV), torch.empty((Q, k), dtype=torch.int32, device=DEV)
    rng = torch.zeros(2, dtype=torch.int32, device=DEV)
    qd, gd, sd = _dev(q, np.float32), _dev(g, np.float32), _dev(skip, np.int32)
    assert lib.fn_gallery_search(_ptr(qd), Q, _ptr(gd), Gn, q.shape[1], k, metric, _ptr(sd), None, 0, _ptr(ws), _ptr(dist), _ptr(rows), None,
                                 _ptr(rng), _stream()) == 0
    return dist.cpu().numpy(), rows.cpu().numpy(), rng.cpu().tolist()


@pytest.mark.parametrize("how", ["random", "kmeans"])
def test_all_lists_probed_equals_the_exhaustive_search(how):
    from facenet_amd.recognize import Gallery
    g, q, assign, _, _ = constructed()
    if how == "kmeans":
        assign = Gallery(g, device=DEV).kmeans(L, iters=3)[1].cpu().numpy()
    probes = np.stack([np.random.default_rng(i).permutation(L) for i in range(70)]).astype(np.int32)
    skip = np.random.default_rng(9).integers(-1, G, 70).astype(np.int32)
    for metric, k, sk in ((0, 5, None), (0, 64, skip), (1, 10, skip), (1, 1, None)):
        dist, rows, words = gpu_gallery_search(q, g, k, metric, sk)
        got = gpu_ivf_search(q, g, assign, L, probes, k, metric=metric, skip=sk)
        assert np.array_equal(got["rows"], rows) and np.array_equal(got["dist"].view(np.uint32), dist.view(np.uint32))      # both metrics: bits
        assert got["range"] == (_decode_ord(words[0]), _decode_ord(words[1]))


def test_argument_rules():
    """Every rule of the C entry points is refused with -1 and a message, without a launch (the pre-filled outputs stay)."""
    lib = _lib.load()

    def refused(got):
        assert got["rc"] == -1 and lib.fn_last_error().decode() != ""
        assert (got["dist"] == FILL_F).all() and (got["rows"] == FILL_I).all()
        return lib.fn_last_error().decode()

    def call(Q=2, Gn=3, Ln=2, En=8, nprobe=1, k=1, metric=0, qoff=0, goff=0, wsoff=0, null=()):
        qd = torch.zeros(64, dtype=torch.float32, device=DEV)
        gd = torch.zeros(64, dtype=torch.float32, device=DEV)
        ws = torch.zeros(4096, dtype=torch.int64, device=DEV)
        dist = torch.full((256,), FILL_F, dtype=torch.float32, device=DEV)
        rows = torch.full((256,), FILL_I, dtype=torch.int32, device=DEV)
        ids = torch.arange(3, dtype=torch.int32, device=DEV)
        ls = torch.tensor([0, 2, 3], dtype=torch.int32, device=DEV)
        pr = torch.zeros(64, dtype=torch.int32, device=DEV)
        ptr = {"queries": qd.data_ptr() + qoff, "lists": gd.data_ptr() + goff, "workspace": ws.data_ptr() + wsoff, "dist": dist.data_ptr(),
               "rows": rows.data_ptr(), "ids": ids.data_ptr(), "list_start": ls.data_ptr(), "probes": pr.data_ptr()}
        ptr.update({name: None for name in null})
        rc = lib.fn_ivf_search(ptr["queries"], Q, ptr["lists"], ptr["ids"], Gn, ptr["list_start"], Ln, En, ptr["probes"], nprobe, k, metric, None,
                               ptr["workspace"], ptr["dist"], ptr["rows"], None, _stream())
        torch.cuda.synchronize()
        return {"rc": rc, "dist": dist.cpu().numpy(), "rows": rows.cpu().numpy()}

    assert call()["rc"] == 0
    for kw in (dict(Q=0), dict(Gn=0), dict(Ln=0), dict(nprobe=0), dict(k=0), dict(k=65), dict(Ln=2 ** 20 + 1), dict(Q=2 ** 27, nprobe=3)):
        refused(call(**kw))
    for En in (0, 2, 6, 516):
        assert "multiple of 4" in refused(call(En=En))
    for metric in (-1, 2):
        assert refused(call(metric=metric)) == f"Undefined similarity metric {metric}"
    assert "16-byte aligned" in refused(call(qoff=4))
    assert "16-byte aligned" in refused(call(goff=8))
    assert "16-byte aligned" in refused(call(wsoff=8))
    for name in ("queries", "lists", "workspace", "dist", "rows", "ids", "list_start", "probes"):
        assert "bad arguments" in refused(call(null=(name,)))

    def update(N=3, Ln=2, En=8, null=(), same=False):
        rows = torch.zeros(64, dtype=torch.float32, device=DEV)
        prev = torch.zeros(64, dtype=torch.float32, device=DEV)
        out = torch.full((64,), FILL_F, dtype=torch.float32, device=DEV)
        kept = torch.full((8,), FILL_I, dtype=torch.int32, device=DEV)
        order = torch.arange(3, dtype=torch.int32, device=DEV)
        ls = torch.tensor([0, 2, 3], dtype=torch.int32, device=DEV)
        ptr = {"rows": rows.data_ptr(), "order": order.data_ptr(), "list_start": ls.data_ptr(), "prev": prev.data_ptr(),
               "centroids": prev.data_ptr() if same else out.data_ptr(), "kept": kept.data_ptr()}
        ptr.update({name: None for name in null})
        rc = lib.fn_kmeans_update(ptr["rows"], N, En, ptr["order"], ptr["list_start"], Ln, ptr["prev"], ptr["centroids"], ptr["kept"], _stream())
        torch.cuda.synchronize()
        if rc != 0:
            assert rc == -1 and (out == FILL_F).all() and (kept == FILL_I).all()
        return rc, lib.fn_last_error().decode()

    assert update()[0] == 0
    for kw in (dict(N=0), dict(Ln=0), dict(same=True)):
        rc, text = update(**kw)
        assert rc == -1 and text != ""
    for En in (0, 6, 516):
        assert "multiple of 4" in update(En=En)[1]
    for name in ("rows", "order", "list_start", "prev", "centroids", "kept"):
        rc, text = update(null=(name,))
        assert rc == -1 and "bad arguments" in text


# ---- Gallery.kmeans and IVFGallery -----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def blob_gallery():
    return vo.blobs(600, E, 12, seed=5, spread=0.6)


def test_gallery_kmeans_follows_the_oracle():
    from facenet_amd.recognize import Gallery
    rows = blob_gallery()
    gal = Gallery(rows, device=DEV)
    for iters in (1, 2, 3, 4, 5):                              # the state after every iteration
        want_c, want_a, want_info = vo.kmeans(rows, 12, iters=iters, seed=7)
        cents, assign, info = gal.kmeans(12, iters=iters, seed=7)
        assert cents.is_cuda and assign.is_cuda and assign.dtype == torch.int32 and tuple(cents.shape) == (12, E)
        assert np.array_equal(cents.cpu().numpy().view(np.uint32), want_c.view(np.uint32)) and np.array_equal(assign.cpu().numpy(), want_a)
        assert info == want_info
    again = gal.kmeans(12, iters=5, seed=7)
    assert torch.equal(again[0].view(torch.int32), cents.view(torch.int32)) and torch.equal(again[1], assign) and again[2] == info
    other = gal.kmeans(12, iters=5, seed=8)
    assert not torch.equal(other[0], cents)


def test_kmeans_with_a_list_per_row():
    from facenet_amd.recognize import Gallery
    rows = io.unit_rows(40, 16, 6)
    rows[17] = rows[3]                                          # a duplicate: row 17 joins whichever of the two centroids comes first
    want_c, want_a, want_info = vo.kmeans(rows, 40, iters=3, seed=2)
    cents, assign, info = Gallery(rows, device=DEV).kmeans(40, iters=3, seed=2)
    assert np.array_equal(cents.cpu().numpy().view(np.uint32), want_c.view(np.uint32)) and np.array_equal(assign.cpu().numpy(), want_a)
    assert info == want_info and info["empty"] == 1 and info["converged"]


def index_assignment(index):
    assign = np.empty(index.nrof_images, dtype=np.int64)
    assign[index.ids] = np.repeat(np.arange(index.nlist), np.diff(index.list_start))
    return assign


def test_ivf_gallery_against_the_oracle():
    from facenet_amd.ivf import IVFGallery
    from facenet_amd.recognize import Gallery
    rows = blob_gallery()
    labels = np.arange(600) % 12
    names = {c: f"person{c}" for c in range(12)}
    gal = Gallery(rows, labels=labels, names=names, device=DEV)
    index = gal.ivf(12, iters=4, seed=7)
    assert isinstance(index, IVFGallery) and index.nlist == 12 and index.kmeans_info["iterations"] >= 1
    want_c, want_a, _ = vo.kmeans(rows, 12, iters=4, seed=7)
    assign = index_assignment(index)
    assert np.array_equal(assign, want_a) and np.array_equal(index.centroids.embeddings.cpu().numpy().view(np.uint32), want_c.view(np.uint32))
    q = vo.blobs(40, E, 12, seed=6, spread=0.9)
    s = io.chain_similarities(q, rows)
    for nprobe, k in ((1, 5), (3, 64), (12, 7), (50, 2)):       # 50: clamped to nlist, the exhaustive answer
        probes = io.search(q, want_c, min(nprobe, 12))["rows"]
        ref = vo.ivf_search(q, rows, assign, probes, k, s=s)
        dist, near = index.search(q, k=k, nprobe=nprobe)
        assert isinstance(dist, np.ndarray) and np.array_equal(near, ref["rows"]) and np.array_equal(dist.view(np.uint32), ref["dist"].view(np.uint32))
    exhaustive = gal.search(q, k=2)
    assert np.array_equal(near, exhaustive[1]) and np.array_equal(dist.view(np.uint32), exhaustive[0].view(np.uint32))
    dist_t, near_t = index.search(torch.from_numpy(q).to(DEV), k=2, nprobe=12)
    assert dist_t.is_cuda and near_t.is_cuda and np.array_equal(near_t.cpu().numpy(), near)
    skip = ref["rows"][:, 0].copy()
    assert np.array_equal(index.search(q, k=1, nprobe=12, skip=skip)[1][:, 0], ref["rows"][:, 1])

    probes = io.search(rows, want_c, 2)["rows"]
    loo = vo.ivf_search(rows, rows, assign, probes, 3, skip=np.arange(600))
    dist_t, near_t = index.leave_one_out(3, nprobe=2)
    assert near_t.is_cuda and np.array_equal(near_t.cpu().numpy(), loo["rows"]) and np.array_equal(dist_t.cpu().numpy(), loo["dist"])

    index.nprobe = 2                                            # the default of the searches
    ref = vo.ivf_search(q, rows, assign, io.search(q, want_c, 2)["rows"], 1, s=s)
    d, r = ref["dist"][:, 0], ref["rows"][:, 0]
    closed = [(int(labels[i]), names[int(labels[i])], float(x), int(i)) for x, i in zip(d, r)]
    assert index.identify(q) == closed and index.identify(torch.from_numpy(q).to(DEV), k=3, nprobe=2) == closed
    thr = np.sort(d)[len(d) // 2]
    want = [c if x < thr else (-1, None, c[2], c[3]) for c, x in zip(closed, d)]
    assert any(w[0] == -1 for w in want) and any(w[0] >= 0 for w in want) and index.identify(q, threshold=float(thr)) == want

    bad = q.copy()
    bad[2] = rows[10] * np.float32(1.5)                         # row 10's own list is probed: s = 1.5 is met
    with pytest.raises(ValueError, match="embeddings must be normalized to 1, range"):
        index.search(bad, k=1)
    index.search(bad, k=1, atol=None)

    adversarial = IVFGallery.from_assignment(gal, want_c, constructed()[2][np.arange(600) % G] % 12, nprobe=12)
    dist, near = adversarial.search(q, k=2)                     # any assignment: with every list probed, the exhaustive answer
    assert np.array_equal(near, exhaustive[1]) and np.array_equal(dist.view(np.uint32), exhaustive[0].view(np.uint32))


def test_face_pipeline_identifies_through_an_index(tmp_path):
    """FacePipeline.identify hands the device embeddings to whatever gallery it is given: an IVFGallery with every list probed
    answers as the Gallery it was built from.  The network is a stand-in (pixel statistics of the crop, normalised)."""
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
    index = gal.ivf(4, iters=2)
    want = pipeline.identify(frame, gal)
    got = pipeline.identify(frame, index, nprobe=4)
    assert [b.info() for b, _ in got] == [b.info() for b, _ in want] and [w for _, w in got] == [w for _, w in want]
    assert all(0 <= w[3] < len(known) for _, w in got)


def test_app_builds_the_index_when_asked(tmp_path):
    """apps/identify.py: with identify.nlist set the gallery of the options is an IVFGallery with the nprobe asked for, and its
    answers at nprobe = nlist are the plain gallery's; without it, a Gallery as before."""
    from facenet_amd.apps import identify as app
    from facenet_amd.ivf import IVFGallery
    rows = blob_gallery()[:200]
    np.savez(tmp_path / "g.npz", embeddings=rows, labels=np.arange(200) % 12)
    base = {"dataset": {"path": str(tmp_path / "photos")}, "gallery": {"path": str(tmp_path / "g.npz")}}
    plain, thr = app.load_gallery(app.load_options(overrides=dict(base, identify={"threshold": 0.5})))
    assert type(plain).__name__ == "Gallery" and thr == np.float32(0.5)
    index, thr = app.load_gallery(app.load_options(overrides=dict(base, identify={"threshold": 0.5, "nlist": 6, "nprobe": 6})))
    assert isinstance(index, IVFGallery) and (index.nlist, index.nprobe) == (6, 6) and thr == np.float32(0.5)
    q = torch.from_numpy(rows[:9]).to(DEV)
    for a, b in zip(index.search(q, k=3), plain.search(q, k=3)):
        assert torch.equal(a, b)
    assert app.load_gallery(app.load_options(overrides=dict(base, identify={"nlist": 1000})))[0].nlist == 200       # one list per row at most
