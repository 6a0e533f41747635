"""The pair-classifier kernels on inputs whose distances are exact (tests/pair_lattice.py; DESIGN.md section 16, "Exact counts"):
fn_f2f_pair_counts on classes larger than one 64-row tile with the threshold ON attainable distances, fn_f2f_distance across exact
tile boundaries bit for bit, fn_f2f_row_norms at its row and lane tails, and the loss kernel with an embedding size that is no
multiple of the 16-element stage.  Lattice rows have norm exactly 1, so d = 2 (1 - dot) exactly in both modes whatever theta is."""
import functools

import numpy as np
import pytest
import torch

from facenet_amd import _lib
from tests import faceclass_oracle as fo
from tests import pair_lattice as pl

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 8
FILL_F, FILL_L = -77.0, 0x5A5A5A5A5A5A
MODES = [fo.MODE_DISTANCE, fo.MODE_NORMALIZED]
ALPHA, THETA = 7.0, 0.8
FORMS = [(64, 0), (16, 4), (16, 20), (4, 0)]           # (E0, E_pad): E = 64, 20, 36 (a partial 16-element stage) and 4


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def run_norms(x):
    lib = _lib.load()
    n, E = x.shape
    xd = _dev(x, np.float32)
    out = torch.full((n + GUARD,), FILL_F, dtype=torch.float32, device=DEV)
    assert lib.fn_f2f_row_norms(xd.data_ptr(), n, E, out.data_ptr(), _stream()) == 0, lib.fn_last_error()
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert (o[n:] == FILL_F).all()
    return o[:n]


def _norms_for(x, mode):
    """Device norms for the distance mode (they must be exactly 1 on lattice rows); none in the normalized mode."""
    if mode == fo.MODE_NORMALIZED:
        return None
    n = run_norms(x)
    return _dev(n, np.float32)


def _params(threshold):
    return _dev(np.array([ALPHA, threshold, THETA, 0.0]), np.float32)


def run_counts(table, starts, mode, threshold):
    lib = _lib.load()
    C = len(starts) - 1
    slots = C * (C + 1) // 2
    td, sd, nd, pd = _dev(table, np.float32), _dev(starts, np.int32), _norms_for(table, mode), _params(threshold)
    out = torch.full((slots + GUARD,), FILL_L, dtype=torch.int64, device=DEV)
    rc = lib.fn_f2f_pair_counts(td.data_ptr(), None if nd is None else nd.data_ptr(), sd.data_ptr(), C, table.shape[1], mode, pd.data_ptr(),
                                out.data_ptr(), _stream())
    assert rc == 0, lib.fn_last_error()
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert (o[slots:] == FILL_L).all()
    return o[:slots]


def run_distance(x, y, mode, threshold, logits):
    lib = _lib.load()
    (N, E), M = x.shape, y.shape[0]
    xd, yd, nx, ny, pd = _dev(x, np.float32), _dev(y, np.float32), _norms_for(x, mode), _norms_for(y, mode), _params(threshold)
    out = torch.full((N * M + GUARD,), FILL_F, dtype=torch.float32, device=DEV)
    rc = lib.fn_f2f_distance(xd.data_ptr(), None if nx is None else nx.data_ptr(), N, yd.data_ptr(), None if ny is None else ny.data_ptr(), M, E,
                             mode, pd.data_ptr(), logits, out.data_ptr(), _stream())
    assert rc == 0, lib.fn_last_error()
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert (o[N * M:] == FILL_F).all()
    return o[:N * M].reshape(N, M)


# ---- fn_f2f_pair_counts ---------------------------------------------------------------------------------------------------------
COUNT_SIZES = [1, 63, 64, 65, 130]                      # one, two and three 64-row tiles per side


@functools.lru_cache(maxsize=None)
def count_case(E0, E_pad):
    emb, starts, H = pl.lattice_classes(COUNT_SIZES, seed=21, flips=E0 // 2, E_pad=E_pad, E0=E0)
    one, two = np.float32(1.0), np.float32(2.0)
    thr = np.array([one, np.nextafter(one, np.float32(9)), two, np.nextafter(two, np.float32(9))], np.float32)
    counts, P = pl.exact_counts(H, starts, thr, 0, E0, full=True)
    # the threshold is decided on real pairs: in every class pair but those of the one-row class some distance sits on 1 or on 2
    on = (counts[:, 1] - counts[:, 0]) + (counts[:, 3] - counts[:, 2])
    assert np.count_nonzero(on) >= 10 and np.array_equal(P, np.outer(COUNT_SIZES, COUNT_SIZES)[np.tril_indices(5)])
    return emb, starts, thr, counts


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("E0,E_pad", FORMS)
def test_pair_counts_on_and_just_above_attainable_distances(E0, E_pad, mode):
    emb, starts, thr, counts = count_case(E0, E_pad)
    if mode == fo.MODE_DISTANCE:
        assert np.array_equal(run_norms(emb), np.ones(len(emb), np.float32))
    for n, t in enumerate(thr):
        got = run_counts(emb, starts, mode, t)
        assert np.array_equal(got, counts[:, n]), (float(t), got, counts[:, n])         # no allowance


# ---- fn_f2f_distance --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("E0,E_pad", FORMS)
@pytest.mark.parametrize("N,M", [(64, 64), (65, 63), (1, 129), (130, 1)])
def test_distance_and_logits_bit_for_bit(N, M, E0, E_pad, mode):
    x, _, _ = pl.lattice_classes([N], seed=N, flips=E0 // 2, E_pad=E_pad, E0=E0)
    y, _, _ = pl.lattice_classes([M], seed=1000 + M, flips=E0 // 2, E_pad=E_pad, E0=E0)
    h = (E0 - np.sign(x[:, :E0]).astype(np.int64) @ np.sign(y[:, :E0]).astype(np.int64).T) // 2
    want = (4.0 * h / E0).astype(np.float32)                                          # h / 16 at E0 = 64: exact
    assert np.array_equal(want.astype(np.float64), 4.0 * h / E0)
    got = run_distance(x, y, mode, 1.1, 0)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    thr = np.float32(1.1)
    want_logits = np.float32(ALPHA) * (thr - want)                                    # two fp32 roundings, as the kernel spells them
    assert want_logits.dtype == np.float32
    got = run_distance(x, y, mode, 1.1, 1)
    assert np.array_equal(got.view(np.uint32), want_logits.view(np.uint32))


# ---- fn_f2f_row_norms -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", [4, 20, 64, 100])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 9])
def test_row_norms_within_one_ulp(n, E):
    """Four rows per workgroup, 64 lanes per row: n around 4 and E below, at and above 64.  fp64 sum, one rounding."""
    rng = np.random.default_rng(100 * n + E)
    x = (rng.standard_normal((n, E)) * rng.uniform(0.1, 3.0, (n, 1))).astype(np.float32)
    want = np.sqrt((x.astype(np.float64) ** 2).sum(axis=1))
    got = run_norms(x)
    assert np.all(np.abs(got.astype(np.float64) - want) <= np.spacing(want.astype(np.float32)).astype(np.float64))
    E0 = {4: 4, 20: 16, 64: 64, 100: 64}[E]
    lat, _, _ = pl.lattice_classes([n], seed=n, flips=E0 // 2, E_pad=E - E0, E0=E0)
    assert np.array_equal(run_norms(lat), np.ones(n, np.float32))


# ---- fn_f2f_pair_loss_fwd_bwd -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("E", [20, 36])
@pytest.mark.parametrize("P,K", [(32, 2), (13, 5)])
def test_loss_with_a_partial_embedding_stage(P, K, E, mode):
    """P K = 64 (exactly one tile) and 65 (one row in the second tile); E % 16 != 0 takes load_row4's zero padding."""
    lib = _lib.load()
    embs = fo.clustered([K + 2] * P, E, seed=P + E)
    if mode == fo.MODE_NORMALIZED:
        embs = [(e / np.linalg.norm(e, axis=1, keepdims=True)).astype(np.float32) for e in embs]
    table = np.concatenate(embs)
    rng = np.random.default_rng(P * K)
    rows = np.concatenate([c * (K + 2) + rng.permutation(K + 2)[:K] for c in rng.permutation(P)]).astype(np.int32)
    B = P * K
    nt = -(-B // 64)
    tiles = nt * (nt + 1) // 2
    q = fo.pos_weight(P, K)
    td, nd, rd, pd = _dev(table, np.float32), _norms_for(table, mode), _dev(rows, np.int32), _params(1.1)
    ws = torch.full((4 * tiles + GUARD,), FILL_F, dtype=torch.float64, device=DEV)
    loss = torch.full((1 + GUARD,), FILL_F, dtype=torch.float32, device=DEV)
    grad = torch.full((4 + GUARD,), FILL_F, dtype=torch.float32, device=DEV)
    rc = lib.fn_f2f_pair_loss_fwd_bwd(td.data_ptr(), None if nd is None else nd.data_ptr(), len(table), rd.data_ptr(), P, K, E, mode, q, pd.data_ptr(),
                                      loss.data_ptr(), grad.data_ptr(), ws.data_ptr(), 4 * tiles, _stream())
    assert rc == 0, lib.fn_last_error()
    torch.cuda.synchronize()
    loss, grad, ws = loss.cpu().numpy(), grad.cpu().numpy(), ws.cpu().numpy()
    assert (loss[1:] == FILL_F).all() and (grad[4:] == FILL_F).all() and (ws[4 * tiles:] == FILL_F).all()
    want_loss, want_grad, scale = fo.pair_loss(table[rows], P, K, mode, ALPHA, 1.1, THETA, q=q)
    # the tolerances of test_gpu_faceclass.py::test_loss_and_gradients_match_the_oracle
    assert abs(loss[0] - want_loss) <= 1e-4 * abs(want_loss), (loss[0], want_loss)
    for j in range(3):
        assert abs(grad[j] - want_grad[j]) <= 1e-4 * max(abs(want_grad[j]), scale[j] * 1e-2) + 1e-12, (j, grad[j], want_grad[j])
    assert grad[3] == 0.0 and (mode == fo.MODE_DISTANCE or grad[2] == 0.0)
