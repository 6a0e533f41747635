"""fn_gallery_candidates / Gallery.candidates / Gallery.templates on the MI355X against the NumPy oracle
(tests/candidates_oracle.py): rows and metric-0 distances bit for bit, metric-1 distances within the 8 * 2^-24 relative bound of
tests/test_gpu_identify.py, tails -1 / +inf, range = the min / max of the chain values.  Column 0 of every result is compared
with fn_gallery_search at k = 1.  Output buffers are over-allocated and pre-filled, so a write past [Q, k] is seen."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from facenet_amd import _lib
from facenet_amd.statistics import _decode_ord, cmc
from tests import candidates_oracle as co
from tests import identify_oracle as io
from tests import ivf_oracle
from tests.opensearch_oracle import ragged_labels
from tests.test_gpu_identify import gpu_search

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 7                      # extra words behind every output buffer
FILL_F, FILL_I = -77.0, -77


def _dev(a, dtype):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def _ptr(t):
    return None if t is None else t.data_ptr()


def gpu_candidates(q, g, labels, k, metric=0, skip=None, slab_rows=0, want_range=True):
    """One fn_gallery_candidates call -> dict(rc, dist, rows, range (lo, hi) floats); the guard words are checked here."""
    lib = _lib.load()
    Q, G, E = q.shape[0], g.shape[0], q.shape[1]
    nbytes = C.c_longlong(-1)
    rc = lib.fn_gallery_candidates_workspace(Q, G, k, slab_rows, C.byref(nbytes))
    assert rc == 0 and nbytes.value >= Q * k * 8 and nbytes.value % (Q * k * 8) == 0
    ws = torch.full((nbytes.value // 8 + GUARD,), 0x5A5A5A5A5A5A, dtype=torch.int64, device=DEV)
    n = Q * k
    dist = torch.full((n + GUARD,), FILL_F, dtype=torch.float32, device=DEV)
    rows = torch.full((n + GUARD,), FILL_I, dtype=torch.int32, device=DEV)
    rng = torch.zeros(2 + GUARD, dtype=torch.int32, device=DEV) if want_range else None
    qd, gd, sd, ld = _dev(q, np.float32), _dev(g, np.float32), _dev(skip, np.int32), _dev(labels, np.int32)
    rc = lib.fn_gallery_candidates(_ptr(qd), Q, _ptr(gd), G, _ptr(ld), E, k, metric, _ptr(sd), slab_rows, _ptr(ws), _ptr(dist), _ptr(rows),
                                   _ptr(rng), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = {"rc": rc, "dist": dist.cpu().numpy(), "rows": rows.cpu().numpy()}
    if rc != 0:
        return out
    assert (out["dist"][n:] == FILL_F).all() and (out["rows"][n:] == FILL_I).all()
    assert (ws[nbytes.value // 8:] == 0x5A5A5A5A5A5A).all()
    out["dist"], out["rows"] = out["dist"][:n].reshape(Q, k), out["rows"][:n].reshape(Q, k)
    if rng is not None:
        words = rng.cpu().tolist()
        assert words[2:] == [0] * GUARD
        out["range"] = (_decode_ord(words[0]), _decode_ord(words[1]))
    return out


def check(got, ref, metric=0):
    """The checker of every result: rows equal, metric-0 distances bit for bit, metric-1 distances within 8 * 2^-24 relative of the
    float64 arccos, tails -1 / +inf, range = min / max of the chain."""
    assert got["rc"] == 0
    assert np.array_equal(got["rows"], ref["rows"])
    ok = ref["rows"] >= 0
    assert (got["rows"][~ok] == -1).all() and np.isposinf(got["dist"][~ok]).all()
    if metric == 0:
        assert np.array_equal(got["dist"].view(np.uint32), ref["dist"].view(np.uint32))          # bit for bit
    else:
        err = np.abs(got["dist"][ok].astype(np.float64) - ref["dist"][ok])
        assert (err <= 8 * 2.0 ** -24 * np.abs(ref["dist"][ok])).all(), err.max()
    if "range" in got:
        assert got["range"] == (float(ref["s"].min()), float(ref["s"].max()))


def same_arrays(a, b):
    return np.array_equal(a["rows"], b["rows"]) and np.array_equal(a["dist"].view(np.uint32), b["dist"].view(np.uint32))


def run(q, g, labels, k, metric=0, skip=None, slab_rows=0, s=None):
    """Oracle, one call, the checker, and column 0 against fn_gallery_search at k = 1 -> (got, ref)."""
    ref = co.candidates(q, g, labels, k, metric=metric, skip=skip, s=s)
    got = gpu_candidates(q, g, labels, k, metric=metric, skip=skip, slab_rows=slab_rows)
    check(got, ref, metric)
    first = gpu_search(q, g, 1, metric=metric, skip=skip, slab_rows=slab_rows)
    assert first["rc"] == 0 and np.array_equal(got["rows"][:, 0], first["rows"][:, 0])
    assert np.array_equal(got["dist"][:, 0].view(np.uint32), first["dist"][:, 0].view(np.uint32)) and got["range"] == first["range"]
    return got, ref


def ragged_sizes(G, seed, largest=8):
    """Class sizes in [1, largest] that add up to G."""
    rng, sizes = np.random.default_rng(seed), []
    while sum(sizes) < G:
        sizes.append(min(int(rng.integers(1, largest + 1)), G - sum(sizes)))
    return sizes


def class_rows(labels, E, seed, spread=0.6):
    """Unit rows around one random centre per label: a probe's nearest rows are mostly, not only, its own identity's."""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((int(np.max(labels)) + 1, E))
    centres /= np.linalg.norm(centres, axis=1, keepdims=True)
    x = centres[labels] + spread * rng.standard_normal((len(labels), E)) / np.sqrt(E)
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


SHAPES = [(1, 1, 4, 1), (1, 63, 40, 5), (17, 65, 72, 64), (65, 300, 512, 10), (64, 129, 128, 1)]


@functools.lru_cache(maxsize=None)
def shape_case(Q, G, E):
    q, g = io.unit_rows(Q, E, 1000 + Q), io.unit_rows(G, E, 2000 + G)
    return q, g, io.chain_similarities(q, g)


@pytest.mark.parametrize("shuffled", [False, True])
@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("Q,G,E,k", SHAPES)
def test_shapes(Q, G, E, k, metric, shuffled):
    """Ragged query and gallery tiles, a ragged E chunk, k at its limit (more than the identities: the tail), classes of 1 .. 8
    rows, contiguous as class directories are and shuffled."""
    q, g, s = shape_case(Q, G, E)
    labels = ragged_labels(ragged_sizes(G, G), seed=G if shuffled else None)
    got, ref = run(q, g, labels, k, metric=metric, s=s)
    classes = len(np.unique(labels))
    assert ((got["rows"] >= 0).sum(axis=1) == min(k, classes)).all()
    for row in got["rows"]:
        found = labels[row[row >= 0]]
        assert len(set(found.tolist())) == len(found)            # distinct identities


@pytest.mark.parametrize("metric", [0, 1])
def test_degenerate_labelings(metric):
    q, g, s = shape_case(17, 65, 72)
    for k in (1, 7, 64):                                       # every row its own identity: fn_gallery_search's arrays, bit for bit
        got, _ = run(q, g, np.arange(65), k, metric=metric, s=s)
        assert same_arrays(got, gpu_search(q, g, k, metric=metric))
    got, _ = run(q, g, np.full(65, 3), 5, metric=metric, s=s)       # one identity: one candidate, then the tail
    first = gpu_search(q, g, 1, metric=metric)
    assert same_arrays({"rows": got["rows"][:, :1], "dist": got["dist"][:, :1]}, first)
    assert (got["rows"][:, 1:] == -1).all() and np.isposinf(got["dist"][:, 1:]).all()
    got, _ = run(q, g, np.arange(65) % 3, 5, metric=metric, s=s)    # fewer identities than k
    assert (got["rows"][:, :3] >= 0).all() and (got["rows"][:, 3:] == -1).all()


def test_one_identity_floods_the_list():
    """A class of 300 rows nearer to the probes than 100 singletons.  The 64 nearest rows are one person, which is the gap this
    search closes: the candidate list names 16 people."""
    q, g = io.adversarial_order(400, 64, 5)                    # rows ascend towards query 0: the last 300 are the nearest
    labels = np.concatenate([1 + np.arange(100), np.zeros(300, dtype=np.int64)])
    rows64 = gpu_search(q, g, 64)["rows"]
    assert (labels[rows64] == 0).all()                         # search(k = 64): a single label in every column
    got, ref = run(q, g, labels, 16)
    found = labels[got["rows"]]
    assert (found[:, 0] == 0).all() and all(len(set(row.tolist())) == 16 for row in found)
    assert np.array_equal(found, ref["labels"])
    run(q, g, labels, 16, slab_rows=128)


@pytest.mark.parametrize("k", [5, 64])
def test_the_cut_runs_on_every_tile(k):
    """Every row is nearer than all before it, so every column tile beats every threshold; labels that recur every 37 rows (most
    entries of a list are dominated by a later one), in runs of 9 (an identity's rows are adjacent columns of a tile, across tile
    and slab ends), every 3 rows (equal labels within a tile that are not adjacent) and in runs of 2 that recur every 10 rows."""
    q, g = io.adversarial_order(500, 64, 11)
    s = io.chain_similarities(q, g)
    for labels in (np.arange(500) % 37, np.arange(500) // 9, np.arange(500) % 3, np.arange(500) // 2 % 5):
        got, _ = run(q, g, labels, k, s=s)
        assert same_arrays(got, gpu_candidates(q, g, labels, k, slab_rows=128))
    assert got["rows"][0, 0] == 499
    run(q, g[::-1].copy(), np.arange(500) // 9, k)             # the nearest row of a run is its first: the other side of the run minimum


def test_split_mode_and_two_slabs():
    """Q = 16 (the waves split the column tiles, four lists per slab) and Q = 17 at G = 150 in two slabs."""
    g = io.unit_rows(150, 36, 72)
    labels = ragged_labels(ragged_sizes(150, 7), seed=8)
    nbytes = C.c_longlong()
    lib = _lib.load()
    assert lib.fn_gallery_candidates_workspace(16, 150, 7, 128, C.byref(nbytes)) == 0 and nbytes.value == 2 * 4 * 16 * 7 * 8
    assert lib.fn_gallery_candidates_workspace(17, 150, 7, 128, C.byref(nbytes)) == 0 and nbytes.value == 2 * 1 * 17 * 7 * 8
    for Q in (16, 17):
        q = io.unit_rows(Q, 36, 71)
        skip = np.arange(Q, dtype=np.int32) * 9
        results = [run(q, g, labels, 7, skip=skip, slab_rows=slab_rows)[0] for slab_rows in (128, 0)]
        assert same_arrays(*results)


def test_eleven_slabs_through_the_merge():
    """G = 700 in slabs of 64 rows at k = 64: eleven lists of 64 keys per query, more than the merge list holds, with every
    identity's rows spread over the slabs; the library's own slab height returns identical arrays."""
    q, g = io.unit_rows(20, 32, 81), io.unit_rows(700, 32, 82)
    labels = ragged_labels(ragged_sizes(700, 9), seed=10)
    assert len(np.unique(labels)) > 128
    nbytes = C.c_longlong()
    assert _lib.load().fn_gallery_candidates_workspace(20, 700, 64, 64, C.byref(nbytes)) == 0 and nbytes.value == 11 * 20 * 64 * 8
    assert _lib.load().fn_gallery_candidates_workspace(20, 700, 64, 1, C.byref(nbytes)) == 0 and nbytes.value == 11 * 20 * 64 * 8
    s = io.chain_similarities(q, g)
    for metric in (0, 1):
        many, _ = run(q, g, labels, 64, metric=metric, slab_rows=64, s=s)
        one, _ = run(q, g, labels, 64, metric=metric, s=s)
        assert same_arrays(many, one)
    few = labels % 40                                          # 40 identities, each in every slab: the merge meets each eleven times
    assert same_arrays(run(q, g, few, 64, slab_rows=64, s=s)[0], run(q, g, few, 64, s=s)[0])


def test_exact_ties_go_to_the_lower_row():
    """The +-1/8 pool: equal rows inside one identity and in two identities, on both sides of a slab boundary."""
    pool = io.tie_pool(200, 3)
    q = pool[:5].copy()
    g = pool[5:].copy()                                        # 195 rows
    labels = np.arange(195) // 3                               # rows 63, 64, 65 are identity 21
    g[63] = g[64] = q[0]                                       # one identity, both at distance 0 of query 0, across the boundary
    g[130] = q[0]                                              # another identity at the same distance: the lower row's identity first
    g[7] = g[190] = q[1]                                       # two identities at distance 0 of query 1
    labels[100] = labels[7]                                    # ... and a far row of the first of them
    g[150] = g[20]                                             # equal rows of two identities somewhere in the middle
    for k in (1, 2, 3, 10):
        results = [run(q, g, labels, k, slab_rows=sr) for sr in (64, 128, 0)]
        assert same_arrays(results[0][0], results[1][0]) and same_arrays(results[0][0], results[2][0])
    got = results[0][0]
    assert got["rows"][0, :2].tolist() == [63, 130] and got["dist"][0, :2].tolist() == [0.0, 0.0]
    assert got["rows"][1, :2].tolist() == [7, 190]
    _, d0 = io.distances(results[0][1]["s"])
    assert any(len(np.unique(d0[i])) < 150 for i in range(5))   # the pool does tie


def test_skip_and_leave_one_out():
    sizes = ragged_sizes(200, 21)
    labels = ragged_labels(sizes, seed=22)
    assert 1 in sizes and len(sizes) <= 64
    pool = class_rows(labels, 24, 23)
    skip = np.arange(200, dtype=np.int32)
    k = len(sizes)                                             # every identity there is
    got, _ = run(pool, pool, labels, k, skip=skip)
    assert (got["rows"] != skip[:, None]).all()                # never the probe's own row
    found = np.where(got["rows"] >= 0, labels[np.maximum(got["rows"], 0)], -1)
    alone = np.bincount(labels)[labels] == 1
    own = (found == labels[:, None]).any(axis=1)
    assert (own == ~alone).all()                               # its identity whenever that has another row; a skipped only row removes it
    assert ((got["rows"] >= 0).sum(axis=1) == k - alone).all()
    none, _ = run(pool, pool, labels, 4, skip=np.full(200, -1, np.int32))
    plain, _ = run(pool, pool, labels, 4)
    assert same_arrays(none, plain) and (plain["rows"][:, 0] == skip).all()    # without skip every row finds itself first


def test_identity_level_cmc():
    """statistics.cmc of leave_one_out_candidates' rows is the curve of the brute-force identity ranks, and never below the
    row-level curve of leave_one_out."""
    from facenet_amd.recognize import Gallery
    labels = ragged_labels(ragged_sizes(300, 31, largest=12), seed=32)
    pool = class_rows(labels, 16, 33, spread=2.5)
    gal = Gallery(pool, labels=labels * 5 + 2, device=DEV)                       # (any non-negative labels)
    dist, rows, found = gal.leave_one_out_candidates(20)
    assert dist.is_cuda and rows.dtype == torch.int32 and found.dtype == torch.int64 and tuple(found.shape) == (300, 20)
    ref = co.candidates(pool, pool, labels, 20, skip=np.arange(300))
    assert np.array_equal(rows.cpu().numpy(), ref["rows"]) and np.array_equal(dist.cpu().numpy(), ref["dist"])
    assert np.array_equal(found.cpu().numpy(), np.where(ref["labels"] >= 0, ref["labels"] * 5 + 2, -1))
    curve, left_out = cmc(gal.labels, rows.cpu().numpy())
    ranks = co.identity_ranks(pool, labels, pool, labels, skip=np.arange(300), s=ref["s"])
    scored = ranks >= 0
    assert left_out == int((~scored).sum()) > 0
    want = np.array([np.count_nonzero(ranks[scored] <= r) / scored.sum() for r in range(20)], dtype=np.float64)
    assert np.array_equal(curve, want) and 0 < curve[0] < curve[-1]
    row_curve, _ = cmc(gal.labels, gal.leave_one_out(20)[1].cpu().numpy())
    assert (curve >= row_curve).all() and (curve > row_curve).any()


def test_argument_rules():
    """Every rule of the C ABI is refused with a message and without a launch (the pre-filled outputs stay as they were)."""
    lib = _lib.load()

    def refused(got):
        assert got["rc"] == -1 and lib.fn_last_error().decode() != ""
        assert (got["dist"] == FILL_F).all() and (got["rows"] == FILL_I).all()
        return lib.fn_last_error().decode()

    def call(Q=2, G=3, E=8, k=1, metric=0, qoff=0, goff=0, wsoff=0, slab_rows=0, null=()):
        qd = torch.zeros(64, dtype=torch.float32, device=DEV)
        gd = torch.zeros(64, dtype=torch.float32, device=DEV)
        ws = torch.zeros(1024, dtype=torch.int64, device=DEV)
        dist = torch.full((256,), FILL_F, dtype=torch.float32, device=DEV)
        rows = torch.full((256,), FILL_I, dtype=torch.int32, device=DEV)
        lab = torch.zeros(64, dtype=torch.int32, device=DEV)
        ptr = {"queries": qd.data_ptr() + qoff, "gallery": gd.data_ptr() + goff, "workspace": ws.data_ptr() + wsoff,
               "dist": dist.data_ptr(), "rows": rows.data_ptr(), "labels": lab.data_ptr()}
        ptr.update({name: None for name in null})
        rc = lib.fn_gallery_candidates(ptr["queries"], Q, ptr["gallery"], G, ptr["labels"], E, k, metric, None, slab_rows, ptr["workspace"],
                                       ptr["dist"], ptr["rows"], None, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return {"rc": rc, "dist": dist.cpu().numpy(), "rows": rows.cpu().numpy()}

    assert call()["rc"] == 0
    for kw in (dict(Q=0), dict(G=0), dict(k=0), dict(k=65)):
        refused(call(**kw))
    assert "k must be in [1, 64]" in refused(call(k=65))
    for E in (0, 2, 6, 516):
        assert "multiple of 4" in refused(call(E=E))
    for metric in (-1, 2):
        assert refused(call(metric=metric)) == f"Undefined similarity metric {metric}"
    assert "16-byte aligned" in refused(call(qoff=4))
    assert "16-byte aligned" in refused(call(goff=8))
    assert "16-byte aligned" in refused(call(wsoff=8))                          # a workspace that is not the one the sizer described
    assert "bad arguments" in refused(call(slab_rows=-1))
    for name in ("queries", "gallery", "workspace", "dist", "rows"):
        assert "bad arguments" in refused(call(null=(name,)))
    assert "gallery_labels must be given" in refused(call(null=("labels",)))


def test_templates():
    from facenet_amd.recognize import Gallery
    labels = ragged_labels(ragged_sizes(130, 41), seed=42)
    pool = class_rows(labels, 40, 43)
    names = {int(c) * 3 + 1: f"person{c}" for c in np.unique(labels)}
    gal = Gallery(pool, labels=labels * 3 + 1, names=names, files=[f"{c}/{i}.png" for i, c in enumerate(labels)], metric=1, device=DEV)
    tmpl = gal.templates()
    classes = len(np.unique(labels))
    want, kept = ivf_oracle.kmeans_update(pool, labels, np.zeros((classes, 40), np.float32))
    assert not kept.any()
    assert type(tmpl) is Gallery and tmpl.metric == 1 and tmpl.files is None and tmpl.names == names
    assert np.array_equal(tmpl.labels, np.unique(labels) * 3 + 1) and tmpl.nrof_images == tmpl.nrof_classes == classes
    assert np.array_equal(tmpl.embeddings.cpu().numpy().view(np.uint32), want.view(np.uint32))         # bit for bit
    assert torch.equal(gal.templates().embeddings, tmpl.embeddings)                                    # and again
    dist, rows = tmpl.search(pool, k=2)                        # rows of the template gallery are indexed by label
    assert np.array_equal(rows, io.search(pool, want, 2)["rows"]) and (tmpl.labels[rows[:, 0]] == gal.labels).mean() > 0.9
    assert tmpl.identify(pool[:1])[0][:2] == (int(gal.labels[0]), names[int(gal.labels[0])])
    x = io.unit_rows(5, 8, 44)
    x[3] = -x[1]                                               # a class of two antipodal rows has no direction
    with pytest.raises(ValueError, match="label 7 sum to zero"):
        Gallery(x, labels=[2, 7, 2, 7, 9], device=DEV).templates()


def test_public_path():
    from facenet_amd.faceclass import FaceToFaceNormalizedEmbeddingsClassifier
    from facenet_amd.recognize import Gallery
    labels = ragged_labels(ragged_sizes(90, 51), seed=52)
    g = class_rows(labels, 16, 53)
    names = {int(c): f"person{c}" for c in np.unique(labels)}
    gal = Gallery(g, labels=labels, names=names, device=DEV)
    q = class_rows(labels[:6], 16, 54)
    ref = co.candidates(q, g, labels, 4)
    dist, rows, found = gal.candidates(q, k=4)
    assert all(isinstance(a, np.ndarray) for a in (dist, rows, found)) and (dist.dtype, rows.dtype, found.dtype) == (np.float32, np.int32, np.int64)
    assert np.array_equal(dist, ref["dist"]) and np.array_equal(rows, ref["rows"]) and np.array_equal(found, ref["labels"])
    dist_t, rows_t, found_t = gal.candidates(torch.from_numpy(q).to(DEV), k=4)
    assert dist_t.is_cuda and rows_t.is_cuda and found_t.is_cuda
    assert np.array_equal(dist_t.cpu().numpy(), dist) and np.array_equal(rows_t.cpu().numpy(), rows) and np.array_equal(found_t.cpu().numpy(), found)
    few = gal.candidates(q, k=64)                              # fewer identities than k: -1 labels in the tail
    classes = len(names)
    assert (few[2][:, classes:] == -1).all() and (few[1][:, classes:] == -1).all() and (few[2][:, :classes] >= 0).all()

    closed = [[(int(labels[r]), names[int(labels[r])], float(d), int(r)) for d, r in zip(dq, rq)] for dq, rq in zip(dist, rows)]
    assert gal.identify_candidates(q, 4) == closed and gal.identify_candidates(torch.from_numpy(q).to(DEV), 4) == closed
    thr = dist[0, 2]                                           # exactly one candidate's distance: strict <, so the list stops before it
    want = [[c for c, d in zip(cq, dq) if d < thr] for cq, dq in zip(closed, dist)]
    assert len(want[0]) == 2 and any(len(w) != 2 for w in want)
    assert gal.identify_candidates(q, 4, threshold=float(thr)) == want
    clf = FaceToFaceNormalizedEmbeddingsClassifier(device=DEV)
    clf.params[1] = float(thr)
    assert gal.identify_candidates(q, 4, classifier=clf) == want

    bad = q.copy()
    bad[2] = g[5] * np.float32(1.5)                            # a dot product of about 1.5 with gallery row 5
    s = io.chain_similarities(bad, g)
    with pytest.raises(ValueError, match="embeddings must be normalized to 1, range") as e:
        gal.candidates(bad, k=2)
    assert str(e.value) == "\nembeddings must be normalized to 1, range {} {}".format(float(s.min()), float(s.max()))
    _, rows, _ = gal.candidates(bad, k=2, atol=None)           # the check left out: nothing raised
    assert np.array_equal(rows, co.candidates(bad, g, labels, 2, s=s)["rows"])
