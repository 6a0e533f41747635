"""fn_radius_count / fn_radius_fill / fn_dbscan_* / Gallery.cluster on the MI355X against the NumPy oracle (tests/cluster_oracle.py):
offsets, columns, metric-0 distances, labels and core flags bit for bit, metric-1 distances within the 4-ulp acosf rule (with eps
placed where no pair lies within that band).  Every buffer is over-allocated and pre-filled, so a write past its end is seen."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from facenet_amd import _lib
from facenet_amd.statistics import _decode_ord
from tests import cluster_oracle as co
from tests import identify_oracle as io
from tests.test_gpu_identify_app import detector, photos, pipeline  # noqa: F401  (the fixtures of the identification app's test)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 7
FILL_F, FILL_I, FILL_L = -77.0, -77, 0x5A5A5A5A5A5A


def _dev(a, dtype):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def gpu_radius(q, g, eps, metric=0, skip=None, slab_rows=0, short=0, want_range=True):
    """fn_radius_count, then fn_radius_fill with capacity = nnz - short -> dict(offsets, cols, dist, nnz, range); the guard words
    and, for short > 0, the untouched tail are checked here."""
    lib = _lib.load()
    Q, G, E = q.shape[0], g.shape[0], q.shape[1]
    nbytes = C.c_longlong(-1)
    assert lib.fn_radius_workspace(Q, G, slab_rows, C.byref(nbytes)) == 0 and nbytes.value >= Q * 12 and nbytes.value % (Q * 12) == 0
    words = (nbytes.value + 7) // 8
    ws = torch.full((words + GUARD,), FILL_L, dtype=torch.int64, device=DEV)
    offsets = torch.full((Q + 1 + GUARD,), FILL_L, dtype=torch.int64, device=DEV)
    rng = torch.zeros(2 + GUARD, dtype=torch.int32, device=DEV) if want_range else None
    qd, gd, sd = _dev(q, np.float32), _dev(g, np.float32), _dev(skip, np.int32)
    args = (_ptr(qd), Q, _ptr(gd), G, E, metric, float(np.float32(eps)), _ptr(sd), slab_rows, _ptr(ws))
    assert lib.fn_radius_count(*args, _ptr(offsets), _ptr(rng), _stream()) == 0, lib.fn_last_error()
    off = offsets.cpu().numpy()
    assert (off[Q + 1:] == FILL_L).all()
    off = off[:Q + 1]
    nnz = int(off[Q])
    capacity = max(0, nnz - short)
    cols = torch.full((nnz + GUARD,), FILL_I, dtype=torch.int32, device=DEV)
    dist = torch.full((nnz + GUARD,), FILL_F, dtype=torch.float32, device=DEV)
    assert lib.fn_radius_fill(*args, _ptr(cols), _ptr(dist), capacity, _stream()) == 0, lib.fn_last_error()
    torch.cuda.synchronize()
    cols, dist = cols.cpu().numpy(), dist.cpu().numpy()
    assert (cols[capacity:] == FILL_I).all() and (dist[capacity:] == FILL_F).all()        # nothing at or beyond the capacity
    assert (ws[words:] == FILL_L).all()
    out = {"offsets": off, "cols": cols[:capacity], "dist": dist[:capacity], "nnz": nnz}
    if rng is not None:
        w = rng.cpu().tolist()
        assert w[2:] == [0] * GUARD
        out["range"] = (_decode_ord(w[0]), _decode_ord(w[1]))
    return out


def check_csr(got, ref, metric=0):
    assert np.array_equal(got["offsets"], ref["offsets"])
    assert np.array_equal(got["cols"], ref["cols"])
    if metric == 0:
        assert np.array_equal(got["dist"].view(np.uint32), ref["dist"].view(np.uint32))          # bit for bit
    else:
        err = np.abs(got["dist"].astype(np.float64) - ref["dist"])
        assert (err <= co.ACOS_ULPS * np.abs(ref["dist"])).all(), err.max()
    if "range" in got:
        assert got["range"] == (float(ref["s"].min()), float(ref["s"].max()))


def gpu_dbscan(csr, min_samples, metric=0, emb=None, batch=4):
    """fn_dbscan_init, batches of rounds until the flag is set, fn_dbscan_finish -> (labels, core, info[:4]); guard words checked."""
    lib = _lib.load()
    N = len(csr["offsets"]) - 1
    off, cols, dist = _dev(csr["offsets"], np.int64), _dev(csr["cols"], np.int32), _dev(csr["dist"], np.float32)
    labels, core, ids = (torch.full((N + GUARD,), FILL_I, dtype=torch.int32, device=DEV) for _ in range(3))
    info = torch.full((8 + GUARD,), FILL_I, dtype=torch.int32, device=DEV)
    ed = _dev(emb, np.float32)
    E = 0 if emb is None else emb.shape[1]
    assert lib.fn_dbscan_init(N, _ptr(off), min_samples, _ptr(labels), _ptr(core), _ptr(info), _stream()) == 0, lib.fn_last_error()
    for _ in range(N // batch + 2):                              # N rounds are more than any method needs
        assert lib.fn_dbscan_rounds(N, _ptr(off), _ptr(cols), _ptr(core), _ptr(labels), _ptr(info), batch, _stream()) == 0, lib.fn_last_error()
        if int(info[0].item()):
            break
    assert int(info[0].item()) == 1
    assert lib.fn_dbscan_finish(N, _ptr(off), _ptr(cols), _ptr(dist), metric, _ptr(ed), E, _ptr(core), _ptr(labels), _ptr(ids), _ptr(info),
                                _stream()) == 0, lib.fn_last_error()
    torch.cuda.synchronize()
    for t in (labels, core, ids):
        assert (t[N:] == FILL_I).all()
    assert (info[8:] == FILL_I).all()
    return labels.cpu().numpy()[:N], core.cpu().numpy()[:N].astype(bool), info.cpu().tolist()[:4]


def check_dbscan(csr, min_samples, **kw):
    labels, core, info = gpu_dbscan(csr, min_samples, **kw)
    want_labels, want_core = co.dbscan(csr["offsets"], csr["cols"], csr["d0"], min_samples)
    assert np.array_equal(core, want_core) and np.array_equal(labels, want_labels)
    assert info[0] == 1 and info[2] == want_labels.max() + 1 and info[3] == np.count_nonzero(want_labels < 0)
    return labels, core, info


# ---- radius search ------------------------------------------------------------------------------------------------------------
SHAPES = [(1, 1, 4), (16, 63, 36), (17, 65, 128), (65, 300, 512), (130, 64, 36)]


@functools.lru_cache(maxsize=None)
def shape_case(Q, G, E):
    """(q, g, s, {metric: eps}): eps at about the 0.3 quantile of the distances; metric 1 in a gap of the arccos values."""
    q, g = io.unit_rows(Q, E, 3000 + Q), io.unit_rows(G, E, 4000 + G)
    s = io.chain_similarities(q, g)
    _, d0 = io.distances(s)
    eps0 = np.float32(np.sort(d0.ravel())[int(0.3 * (d0.size - 1))]) if d0.size > 1 else np.float32(d0.max() * 2 + 0.1)
    return q, g, s, {0: eps0, 1: co.metric1_eps(q, g, 0.3, s=s)}


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("Q,G,E", SHAPES)
def test_radius_shapes(Q, G, E, metric):
    """Ragged query and gallery tiles, ragged E chunks, more than one query tile; eps at an attained distance for metric 0."""
    q, g, s, eps = shape_case(Q, G, E)
    ref = co.radius(q, g, eps[metric], metric=metric, s=s)
    assert Q * G == 1 or 0 < ref["offsets"][-1] < Q * G
    check_csr(gpu_radius(q, g, eps[metric], metric=metric), ref, metric)


def test_radius_slabs():
    """slab_rows = 64 at G = 300: five slabs.  The CSR is the one-slab CSR: columns ascend across the slab boundaries."""
    q, g, s, eps = shape_case(65, 300, 512)
    nbytes = C.c_longlong()
    assert _lib.load().fn_radius_workspace(65, 300, 64, C.byref(nbytes)) == 0 and nbytes.value == 5 * 65 * 12
    assert _lib.load().fn_radius_workspace(65, 300, 1, C.byref(nbytes)) == 0 and nbytes.value == 5 * 65 * 12
    for metric in (0, 1):
        ref = co.radius(q, g, eps[metric], metric=metric, s=s)
        many, one = gpu_radius(q, g, eps[metric], metric=metric, slab_rows=64), gpu_radius(q, g, eps[metric], metric=metric)
        check_csr(many, ref, metric)
        assert np.array_equal(many["offsets"], one["offsets"]) and np.array_equal(many["cols"], one["cols"])
        assert np.array_equal(many["dist"].view(np.uint32), one["dist"].view(np.uint32))
        assert (np.diff(ref["offsets"]) > 64).any()               # some row has neighbours in more than one slab


def test_rows_without_a_neighbour_and_an_empty_result():
    q, g = io.unit_rows(20, 16, 5), io.unit_rows(100, 16, 6)
    s = io.chain_similarities(q, g)
    _, d0 = io.distances(s)
    eps = np.sort(d0.ravel())[15]
    ref = co.radius(q, g, eps, s=s)
    degree = np.diff(ref["offsets"])
    assert ref["offsets"][-1] == 15 and (degree == 0).any() and (degree[:-1] == 0).any() and (degree > 0).any()
    check_csr(gpu_radius(q, g, eps), ref)
    none = gpu_radius(q, g, 0.0)
    assert none["nnz"] == 0 and (none["offsets"] == 0).all()
    check_csr(gpu_radius(q, g, -1.0, metric=1), co.radius(q, g, -1.0, metric=1, s=s), 1)


def test_every_pair_and_no_padding_column():
    """eps = 5 is above every distance, and above the d = 2 of a zero-padded column: nnz = Q G and every row holds 0 .. G - 1."""
    q, g, s, _ = shape_case(65, 300, 512)
    for metric in (0, 1):
        ref = co.radius(q, g, 5.0, metric=metric, s=s)
        assert ref["offsets"][-1] == 65 * 300
        for slab_rows in (0, 64):
            got = gpu_radius(q, g, 5.0, metric=metric, slab_rows=slab_rows)
            check_csr(got, ref, metric)
            assert np.array_equal(got["cols"].reshape(65, 300), np.tile(np.arange(300, dtype=np.int32), (65, 1)))
    one = gpu_radius(q[:1], g[:1], np.inf)                        # a single pair in a 64 x 64 tile of padding
    assert one["offsets"].tolist() == [0, 1] and one["cols"].tolist() == [0]


def test_skip():
    pool = io.unit_rows(70, 24, 21)
    skip = np.arange(70, dtype=np.int32)
    ref = co.self_join(pool, 5.0)
    got = gpu_radius(pool, pool, 5.0, skip=skip)
    check_csr(got, ref)
    assert got["nnz"] == 70 * 69 and (got["cols"].reshape(70, 69) != skip[:, None]).all()
    none, plain = gpu_radius(pool, pool, 5.0, skip=np.full(70, -1, np.int32)), gpu_radius(pool, pool, 5.0)
    assert none["nnz"] == plain["nnz"] == 70 * 70 and np.array_equal(none["cols"], plain["cols"])
    part = np.where(skip % 3 == 0, 69 - skip, -1).astype(np.int32)
    for slab_rows in (0, 64):
        check_csr(gpu_radius(pool, pool, 1.9, skip=part, slab_rows=slab_rows), co.radius(pool, pool, 1.9, skip=part, s=ref["s"]))


def test_strict_comparison_on_exact_ties():
    """The +-1/8 pool: distances are multiples of 1/16, many pairs share one.  eps equal to an attained distance leaves those
    pairs out; the next fp32 up takes them in."""
    pool = io.tie_pool(200, 3)
    q, g = pool[:5], pool[5:]
    s = io.chain_similarities(q, g)
    _, d0 = io.distances(s)
    eps = np.float32(np.median(d0))
    equal = int(np.count_nonzero(d0 == eps))
    assert equal > 5
    below, above = co.radius(q, g, eps, s=s), co.radius(q, g, np.nextafter(eps, np.float32(np.inf)), s=s)
    assert above["offsets"][-1] == below["offsets"][-1] + equal
    for slab_rows in (0, 64):
        check_csr(gpu_radius(q, g, eps, slab_rows=slab_rows), below)
        check_csr(gpu_radius(q, g, np.nextafter(eps, np.float32(np.inf)), slab_rows=slab_rows), above)


def test_capacity_short_of_nnz():
    """capacity = nnz - 5: the entries below it are right, nothing is written at or beyond it (gpu_radius checks the tail)."""
    q, g, s, eps = shape_case(65, 300, 512)
    ref = co.radius(q, g, eps[0], s=s)
    nnz = int(ref["offsets"][-1])
    for slab_rows in (0, 64):
        got = gpu_radius(q, g, eps[0], slab_rows=slab_rows, short=5)
        assert got["nnz"] == nnz and len(got["cols"]) == nnz - 5
        assert np.array_equal(got["cols"], ref["cols"][:nnz - 5]) and np.array_equal(got["dist"], ref["dist"][:nnz - 5])
    assert len(gpu_radius(q, g, eps[0], short=nnz + 3)["cols"]) == 0     # capacity 0: no launch


def test_range_and_normalisation_error():
    from facenet_amd.recognize import Gallery
    q, g = io.unit_rows(4, 16, 41), io.unit_rows(90, 16, 42)
    g[5] = q[2]
    q[2] *= np.float32(1.5)
    s = io.chain_similarities(q, g)
    got = gpu_radius(q, g, 1.0)
    assert got["range"] == (float(s.min()), float(s.max())) and got["range"][1] > 1 + 1e-5
    assert gpu_radius(q, g, 1.0, want_range=False)["nnz"] == got["nnz"]
    gal = Gallery(g, device=DEV)
    with pytest.raises(ValueError, match="embeddings must be normalized to 1, range") as e:
        gal.within(q, 1.0)
    assert str(e.value) == "\nembeddings must be normalized to 1, range {} {}".format(float(s.min()), float(s.max()))
    offsets, rows, dist = gal.within(q, 1.0, atol=None)
    ref = co.radius(q, g, 1.0, s=s)
    assert isinstance(rows, np.ndarray) and np.array_equal(offsets, ref["offsets"]) and np.array_equal(rows, ref["cols"])
    assert np.array_equal(dist, ref["dist"])


@pytest.mark.parametrize("metric", [0, 1])
def test_self_join_is_symmetric(metric):
    x = io.unit_rows(130, 36, 77)
    s = io.chain_similarities(x, x)
    eps = np.float32(1.9) if metric == 0 else co.metric1_eps(x, x, 0.4, s=s)
    got = gpu_radius(x, x, eps, metric=metric, skip=np.arange(130, dtype=np.int32), slab_rows=64)
    check_csr(got, co.self_join(x, eps, metric=metric, s=s), metric)
    rows = np.repeat(np.arange(130), np.diff(got["offsets"]))
    there = {(int(i), int(j)): d for i, j, d in zip(rows, got["cols"], got["dist"].view(np.uint32))}
    assert len(there) > 130 and all(there.get((j, i)) == d for (i, j), d in there.items())


@pytest.mark.parametrize("metric", [0, 1])
def test_agrees_with_the_validation_kernel(metric):
    """A threshold placed exactly on one pair's device distance: the self-join's nnz is twice the pairs fn_confidence_counts bins
    below the same threshold for the same rows (one class: every pair a < b is counted once)."""
    lib = _lib.load()
    n, E = 40, 32
    pool = io.unit_rows(n, E, 51)
    skip = np.arange(n, dtype=np.int32)
    every = gpu_radius(pool, pool, 5.0, metric=metric, skip=skip)
    thr = np.float32(np.sort(every["dist"])[every["nnz"] // 2])
    got = gpu_radius(pool, pool, thr, metric=metric, skip=skip)
    assert got["nnz"] == np.count_nonzero(every["dist"] < thr) and got["nnz"] % 2 == 0 and 0 < got["nnz"] < n * (n - 1)
    assert np.count_nonzero(every["dist"] == thr) >= 2          # the pair itself, from both sides: strict < leaves it out
    emb, cls = _dev(pool, np.float32), _dev(np.array([0, n]), np.int32)
    t_dev = _dev(np.array([thr]), np.float32)
    out = torch.zeros(4, dtype=torch.float64, device=DEV)
    rng = torch.zeros(2, dtype=torch.int32, device=DEV)
    _lib.check(lib.fn_confidence_counts(emb.data_ptr(), cls.data_ptr(), 1, E, t_dev.data_ptr(), 1, metric, out.data_ptr(), rng.data_ptr(),
                                        _stream()))
    pairs = n * (n - 1) // 2
    tp, fn = (out.cpu().numpy()[[0, 3]] * pairs).tolist()
    assert round(tp) + round(fn) == pairs and abs(tp - round(tp)) < 1e-6
    assert 2 * round(tp) == got["nnz"]


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("Q", [16, 17])
def test_search_and_radius_report_the_same_distance_bits(Q, metric):
    """Gallery.search(k = G) against Gallery.within(eps = inf) over the same rows: every query's row -> distance map is the same
    bit for bit.  For metric 1 the search takes the arccos of a scalar fmaf chain, the radius fill that of the MFMA accumulator.
    Q = 16 is the search's split path, Q = 17 its four-wave path with a second, nearly empty 16-row query tile; E = 36 is one
    full 32-chunk and a 4-wide remainder."""
    from facenet_amd.recognize import Gallery
    G, E = 64, 36
    x = np.random.default_rng(20 + Q).standard_normal((G, E))
    x = (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)          # normalised in fp64, then cast
    gal = Gallery(x, metric=metric, device=DEV)
    dist, rows = gal.search(x[:Q], k=G)
    offsets, cols, d = gal.within(x[:Q], np.inf)
    assert offsets.tolist() == [G * i for i in range(Q + 1)] and (np.sort(rows, axis=1) == np.arange(G)).all()
    for i in range(Q):
        from_search = dict(zip(rows[i].tolist(), dist[i].view(np.uint32).tolist()))
        from_radius = dict(zip(cols[G * i:G * (i + 1)].tolist(), d[G * i:G * (i + 1)].view(np.uint32).tolist()))
        assert from_search == from_radius, (i, metric)


def test_radius_argument_rules():
    lib = _lib.load()
    nbytes = C.c_longlong()
    for bad in ((0, 3, 0), (2, 0, 0), (2, 3, -1)):
        assert lib.fn_radius_workspace(*bad, C.byref(nbytes)) == -1 and lib.fn_last_error().decode() != ""
    q = torch.zeros(64, dtype=torch.float32, device=DEV)
    ws = torch.zeros(64, dtype=torch.int64, device=DEV)
    off = torch.full((8,), FILL_L, dtype=torch.int64, device=DEV)

    def count(Q=2, G=3, E=8, metric=0, eps=1.0, qoff=0, slab_rows=0, offsets=off.data_ptr()):
        rc = lib.fn_radius_count(q.data_ptr() + qoff, Q, q.data_ptr(), G, E, metric, eps, None, slab_rows, ws.data_ptr(), offsets, None, _stream())
        torch.cuda.synchronize()
        return rc, lib.fn_last_error().decode()

    for kw, text in ((dict(Q=0), "at least 1"), (dict(G=0), "at least 1"), (dict(E=6), "multiple of 4"), (dict(E=516), "multiple of 4"),
                     (dict(metric=2), "Undefined similarity metric 2"), (dict(eps=float("nan")), "NaN"), (dict(qoff=4), "16-byte aligned"),
                     (dict(slab_rows=-1), "bad arguments"), (dict(offsets=None), "offsets")):
        rc, msg = count(**kw)
        assert rc == -1 and text in msg, (kw, msg)
    assert (off == FILL_L).all()                                 # refused without a launch
    assert count()[0] == 0
    rc = lib.fn_radius_fill(q.data_ptr(), 2, q.data_ptr(), 3, 8, 0, 1.0, None, 0, ws.data_ptr(), None, None, 4, _stream())
    assert rc == -1 and "capacity" in lib.fn_last_error().decode()
    assert lib.fn_dbscan_init(0, off.data_ptr(), 1, off.data_ptr(), off.data_ptr(), off.data_ptr(), _stream()) == -1
    assert lib.fn_dbscan_init(3, off.data_ptr(), 0, off.data_ptr(), off.data_ptr(), off.data_ptr(), _stream()) == -1
    assert lib.fn_dbscan_rounds(3, off.data_ptr(), None, off.data_ptr(), off.data_ptr(), off.data_ptr(), 0, _stream()) == -1
    assert lib.fn_dbscan_finish(3, off.data_ptr(), None, None, 1, None, 0, off.data_ptr(), off.data_ptr(), off.data_ptr(), off.data_ptr(),
                                _stream()) == -1 and "metric 1 needs the embeddings" in lib.fn_last_error().decode()


# ---- DBSCAN -------------------------------------------------------------------------------------------------------------------
def gpu_self_join(x, eps, metric=0, slab_rows=0):
    """The device's self-join CSR, checked against the oracle's, with the oracle's d0 for the oracle's DBSCAN."""
    ref = co.self_join(x, eps, metric=metric)
    got = gpu_radius(x, x, eps, metric=metric, skip=np.arange(len(x), dtype=np.int32), slab_rows=slab_rows)
    check_csr(got, ref, metric)
    got["d0"] = ref["d0"]
    return got


@pytest.mark.parametrize("case", co.BLOB_CASES)
def test_dbscan_blobs(case):
    x, truth, ref = co.blob_case(*case)
    got = gpu_radius(x, x, case[5], skip=np.arange(len(x), dtype=np.int32))
    check_csr(got, ref)
    got["d0"] = ref["d0"]
    labels, core, info = check_dbscan(got, case[6])
    assert info[2] >= case[0] and ((~core & (labels >= 0)).any() == (case[6] > 1))


@pytest.mark.parametrize("N", [1, 63, 64, 65])
def test_dbscan_sizes_and_extremes(N):
    x = io.unit_rows(N, 8, 90 + N)
    every = gpu_self_join(x, 5.0)
    labels, core, info = check_dbscan(every, 1)                  # eps = 5: one cluster
    assert (labels == 0).all() and core.all() and info[2:] == [1, 0]
    labels, core, info = check_dbscan(every, N + 1)              # min_samples above every degree: all noise
    assert (labels == -1).all() and not core.any() and info[2:] == [0, N]
    nobody = gpu_self_join(x, 0.0)
    labels, core, info = check_dbscan(nobody, 1)                 # isolated rows at min_samples = 1: singletons
    assert labels.tolist() == list(range(N)) and info[2:] == [N, 0]
    assert (check_dbscan(nobody, 2)[0] == -1).all()


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("swap", [False, True])
def test_dbscan_bridge_and_tie(swap, metric):
    """tests/test_cluster_host.py's bridge rows: row 0 is at d0 = 1 of both hubs bit for bit and joins the lower row's cluster, row
    11 the nearer hub's.  metric 1 (eps = arccos(0.375), the same graph): the border key is still d0, recomputed on the device."""
    from tests.test_cluster_host import bridge_rows
    x, hub_a = bridge_rows(swap)
    eps = np.float32(1.25) if metric == 0 else np.float32(np.arccos(0.375))
    csr = gpu_self_join(x, eps, metric=metric)
    assert np.array_equal(csr["offsets"], co.self_join(x, 1.25)["offsets"])
    labels, core, _ = check_dbscan(csr, 5, metric=metric, emb=x)
    assert labels[0] == 0 and labels[11] == labels[hub_a] == (0 if swap else 1) and not core[0] and not core[11]


@pytest.mark.parametrize("min_samples", [1, 3])
def test_dbscan_chain(min_samples):
    """1024 rows on a half circle in a seeded permutation, each a neighbour of the next angle only: the graph's diameter is 1023.
    One cluster; at min_samples = 3 the two ends are border rows.  Fewer than N / 8 rounds: propagation from neighbour to
    neighbour, linear in the diameter, does not pass."""
    x = co.chain()
    csr = gpu_self_join(x, 2e-5)
    degree = np.diff(csr["offsets"])
    assert degree.min() == 1 and degree.max() == 2
    labels, core, info = check_dbscan(csr, min_samples, batch=8)
    assert (labels == 0).all() and core.sum() == (1024 if min_samples == 1 else 1022)
    print("rounds", info[1])
    assert 0 < info[1] < 128


# ---- end to end ---------------------------------------------------------------------------------------------------------------
def test_gallery_cluster():
    from facenet_amd.faceclass import FaceToFaceNormalizedEmbeddingsClassifier
    from facenet_amd.recognize import Gallery
    case = co.BLOB_CASES[0]
    x, truth, ref = co.blob_case(*case)
    eps, min_samples = case[5], case[6]
    want_labels, want_core = co.dbscan(ref["offsets"], ref["cols"], ref["d0"], min_samples)
    gal = Gallery(x, device=DEV)
    c = gal.cluster(threshold=eps, min_samples=min_samples)
    assert c.labels.dtype == np.int64 and np.array_equal(c.labels, want_labels) and np.array_equal(c.core, want_core)
    assert c.nrof_clusters == want_labels.max() + 1 and c.nrof_noise == np.count_nonzero(want_labels < 0) and c.rounds >= 1
    assert np.array_equal(c.sizes, np.bincount(want_labels[want_labels >= 0])) and c.sizes.sum() + c.nrof_noise == len(x)
    assert np.array_equal(c.members(2), np.nonzero(want_labels == 2)[0])
    assert c.offsets.is_cuda and np.array_equal(c.offsets.cpu().numpy(), ref["offsets"]) and np.array_equal(c.rows.cpu().numpy(), ref["cols"])
    assert np.array_equal(c.dist.cpu().numpy(), ref["dist"])
    clf = FaceToFaceNormalizedEmbeddingsClassifier(device=DEV)
    clf.params[1] = float(np.float32(eps))
    assert np.array_equal(gal.cluster(classifier=clf, min_samples=min_samples).labels, want_labels)
    with pytest.raises(ValueError, match="metric 0"):
        Gallery(x, metric=1, device=DEV).cluster(classifier=clf)
    # within / neighbours: NumPy in, NumPy out; tensors in, tensors out; max_edges before the rows are allocated
    offsets, rows, dist = gal.within(x[:9], eps, skip=np.arange(9))
    assert isinstance(rows, np.ndarray) and np.array_equal(offsets, ref["offsets"][:10]) and np.array_equal(rows, ref["cols"][:offsets[-1]])
    t_off, t_rows, t_dist = gal.neighbours(eps)
    assert t_off.is_cuda and t_rows.dtype == torch.int32 and t_dist.dtype == torch.float32 and np.array_equal(t_rows.cpu().numpy(), ref["cols"])
    nnz = int(ref["offsets"][-1])
    with pytest.raises(ValueError, match=f"nnz = {nnz} .* max_edges = {nnz - 1}: choose a smaller eps"):
        gal.neighbours(eps, max_edges=nnz - 1)
    assert gal.neighbours(eps, max_edges=nnz)[1].shape == (nnz,)
    # a metric-1 gallery: eps in a gap of the arccos values, the border key still d0
    eps1 = co.metric1_eps(x, x, np.count_nonzero(ref["hit"]) / ref["hit"].size, s=ref["s"])
    ref1 = co.self_join(x, eps1, metric=1, s=ref["s"])
    want1, core1 = co.dbscan(ref1["offsets"], ref1["cols"], ref1["d0"], min_samples)
    assert (~core1 & (want1 >= 0)).any()
    c1 = Gallery(x, metric=1, device=DEV).cluster(threshold=eps1, min_samples=min_samples)
    assert np.array_equal(c1.labels, want1) and np.array_equal(c1.core, core1) and np.array_equal(c1.rows.cpu().numpy(), ref1["cols"])


def _face_clusters(photos):
    """eps at an attained distance between two faces, and the oracle's clustering of the photographs' faces."""
    _, d0 = io.distances(io.chain_similarities(photos.emb, photos.emb))
    off = d0[~np.eye(len(d0), dtype=bool)]
    eps = np.float32(np.sort(off)[len(off) // 2])
    csr = co.self_join(photos.emb, eps)
    return eps, csr, co.dbscan(csr["offsets"], csr["cols"], csr["d0"], 1)[0]


def test_face_pipeline_cluster(pipeline, photos):  # noqa: F811
    eps, csr, want = _face_clusters(photos)
    clustering, faces = pipeline.cluster(photos.frames, threshold=float(eps))
    assert [(i, n) for i, n, _ in faces] == [(i, n) for i, c in enumerate(photos.per_photo) for n in range(c)]
    boxes = [b.info() for frame in photos.frames[:2] for b in pipeline.detector.detect(frame)]
    assert [b.info() for _, _, b in faces] == boxes
    assert np.array_equal(clustering.labels, want) and np.array_equal(clustering.offsets.cpu().numpy(), csr["offsets"])
    assert clustering.core.all() and clustering.nrof_clusters == want.max() + 1
    assert pipeline.cluster(photos.frames[2:], threshold=1.0) == (None, [])


def test_cluster_app(detector, photos, tmp_path):  # noqa: F811
    """`python -m facenet_amd.apps.cluster --config x.yaml` (entered through its click command), from an embeddings file and from
    photographs."""
    import yaml
    from click.testing import CliRunner

    from facenet_amd.apps import cluster as app
    from facenet_amd.statistics import pairwise_clustering_scores
    eps, _, want = _face_clusters(photos)
    n = sum(photos.per_photo)
    cfg, out = tmp_path / "x.yaml", tmp_path / "result" / "c.npz"
    cfg.write_text(yaml.safe_dump({"embeddings": {"path": str(photos.root / "gallery.npz")}, "cluster": {"threshold": float(eps)}, "file": str(out)}))
    result = CliRunner().invoke(app.main, ["--config", str(cfg)], catch_exceptions=False)
    assert result.exit_code == 0, result.output
    z = np.load(out)
    assert sorted(z.files) == ["core", "files", "labels"] and [str(f) for f in z["files"]] == photos.files
    assert z["labels"].dtype == np.int64 and np.array_equal(z["labels"], want) and z["core"].dtype == bool and z["core"].all()
    assert f"number of clusters: {want.max() + 1}" in result.output and "number of noise faces: 0" in result.output
    assert "pairwise precision {:1.5f} recall {:1.5f} F {:1.5f}".format(*pairwise_clustering_scores(photos.labels, want)) in result.output

    cfg.write_text(yaml.safe_dump({"dataset": {"path": str(photos.root / "photos")}, "model": {"normalize": True, "embedding_size": 128},
                                   "image": {"size": 160, "margin": 0.25}, "mtcnn": {"weights_file": detector[1]},
                                   "cluster": {"threshold": float(eps), "min_samples": 1}, "file": str(out)}))
    result = CliRunner().invoke(app.main, ["--config", str(cfg)], catch_exceptions=False)
    assert result.exit_code == 0, result.output
    z = np.load(out)
    assert sorted(z.files) == ["boxes", "core", "face", "files", "labels"] and [str(f) for f in z["files"]] == photos.files
    assert z["face"].tolist() == [i for c in photos.per_photo for i in range(c)] and z["boxes"].shape == (n, 4) and z["boxes"].dtype == np.int64
    assert np.array_equal(z["labels"], want) and "pairwise precision" in result.output
