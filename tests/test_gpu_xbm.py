"""fn_xbm_triplet_fwd_bwd and fn_xbm_enqueue, the cross-batch memory's head in the Trainer and the app on the GPU (DESIGN.md section
32).  The kernel and the fp64 oracle (tests/xbm_oracle.py) both consume the matrices fn_pairwise_sqdist wrote on the device, so every
mining decision is taken on the same bits: a hinge's coef, mcoef, every mpick and info are compared exactly, loss, the soft
coefficients and demb under their derived bounds."""
import os
import socket
import warnings

import numpy as np
import pytest
import torch

from facenet_amd import _lib
from facenet_amd.engine import Network
from facenet_amd.train import Trainer
from oracle import facenet_oracle as fo
from tests import batch_triplet_oracle as bo
from tests import elementwise_oracle as eo
from tests import xbm_oracle as xo
from tests.util import ptr, stream
from tests.util_data import structured_images

pytestmark = pytest.mark.gpu

POISON, TAIL = 7.25, 16


def _rows(n, E, seed, scale=1.5):
    """Rows of norm ``scale``: the kernel must not assume unit norm."""
    x = np.random.default_rng(seed).standard_normal((n, E))
    return (scale * x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(dtype))).cuda()


def _call(lib, x, labels, mem, mem_labels, valid, alpha, soft, with_grad=True, poke=None):
    """One call over poisoned buffers with guard tails -> dict of host arrays (dist, mem_dist: what the device wrote and the kernel
    read; ``poke(dist, mem_dist)`` may edit them on the device in between)."""
    n, E = x.shape
    M = len(mem_labels)
    emb, memt = _dev(x, np.float32), _dev(mem, np.float32)
    dist, mdist = torch.empty(n, n, device="cuda"), torch.empty(n, M, device="cuda")
    _lib.check(lib.fn_pairwise_sqdist(ptr(emb), ptr(emb), ptr(dist), None, n, n, E, 2, stream()))
    _lib.check(lib.fn_pairwise_sqdist(ptr(emb), ptr(memt), ptr(mdist), None, n, M, E, 2, stream()))
    if poke is not None:
        poke(dist, mdist)
    lab, mlab = _dev(labels, np.int32), _dev(mem_labels, np.int32)
    state = _dev([0, valid, 0, 0], np.int32)
    coef = torch.full((n * n + TAIL,), POISON, device="cuda")
    demb = torch.full((n * E + TAIL,), POISON, device="cuda")
    mcoef = torch.full((2 * n + TAIL,), POISON, device="cuda")
    mpick = torch.full((2 * n + TAIL,), 77, dtype=torch.int32, device="cuda")
    loss = torch.full((4,), POISON, device="cuda")
    info = torch.full((8 + TAIL,), 77, dtype=torch.int32, device="cuda")
    before = (memt.clone(), mlab.clone(), state.clone())
    _lib.check(lib.fn_xbm_triplet_fwd_bwd(ptr(emb), ptr(dist), ptr(lab), ptr(memt), ptr(mdist), ptr(mlab), ptr(state),
                                          ptr(demb) if with_grad else None, ptr(loss), ptr(coef), ptr(mpick), ptr(mcoef), ptr(info),
                                          n, M, E, alpha, soft, stream()))
    torch.cuda.synchronize()
    assert bool((coef[n * n:] == POISON).all()) and bool((info[8:] == 77).all()) and bool((demb[n * E:] == POISON).all())
    assert bool((mcoef[2 * n:] == POISON).all()) and bool((mpick[2 * n:] == 77).all())
    for a, b in zip(before, (memt, mlab, state)):                      # the memory is read only (compared as bits: stale rows may be NaN)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    if not with_grad:
        assert bool((demb == POISON).all())
    return dict(dist=dist.cpu().numpy(), mem_dist=mdist.cpu().numpy(), coef=coef[:n * n].view(n, n).cpu().numpy(),
                demb=demb[:n * E].view(n, E).cpu().numpy(), loss=loss.cpu().numpy(), info=info[:8].cpu().numpy(),
                mpick=mpick[:2 * n].view(n, 2).cpu().numpy(), mcoef=mcoef[:2 * n].view(n, 2).cpu().numpy())


def _oracle(got, x, labels, mem, mem_labels, valid, alpha, soft):
    return xo.mine(got["dist"], got["mem_dist"], labels, mem_labels, valid, alpha, soft, emb=x, mem=mem)


def _check(got, o, soft, what, with_grad=True):
    assert np.array_equal(got["info"], o["info"]), (what, got["info"], o["info"])
    assert np.array_equal(got["mpick"], o["mpick"]), what + " mpick"
    if soft:
        eo.check_bound(got["coef"], o["coef"], o["e_coef"], what + " coef")
        eo.check_bound(got["mcoef"], o["mcoef"], o["e_mcoef"], what + " mcoef")
        assert np.array_equal(got["coef"] == 0, o["coef"] == 0) and np.array_equal(got["mcoef"] == 0, o["mcoef"] == 0)
    else:
        assert np.array_equal(got["coef"], o["coef"]), what + " coef"
        assert np.array_equal(got["mcoef"], o["mcoef"]), what + " mcoef"
    print(f"{what}: loss {got['loss'][0]:.9g} fp64 {o['loss']:.12g} bound {o['e_loss']:.3g} info {got['info'].tolist()}")
    eo.check_bound(got["loss"][0], o["loss"], o["e_loss"], what + " loss")
    if with_grad:
        eo.check_bound(got["demb"], o["demb"], o["e_demb"], what + " demb")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- 1. an empty memory is section 31's batch hard ---------------------------------------------------------------------------------
@pytest.mark.parametrize("soft", [0, 1])
@pytest.mark.parametrize("M", [37, 300])
def test_empty_memory_equals_batch_hard_bit_for_bit(lib, M, soft):
    n, E = 37, 67
    x, labels = _rows(n, E, 3), bo.ragged_labels(n, 3)
    mem, mlab = _rows(M, E, 4), np.resize(labels, M)                   # live-looking rows under the batch's own labels, none valid
    got = _call(lib, x, labels, mem, mlab, 0, 0.2, soft)
    emb, lab = _dev(x, np.float32), _dev(labels, np.int32)
    dist = torch.empty(n, n, device="cuda")
    _lib.check(lib.fn_pairwise_sqdist(ptr(emb), ptr(emb), ptr(dist), None, n, n, E, 2, stream()))
    coef, demb = torch.empty(n, n, device="cuda"), torch.empty(n, E, device="cuda")
    loss, info = torch.zeros(4, device="cuda"), torch.zeros(8, dtype=torch.int32, device="cuda")
    _lib.check(lib.fn_batch_triplet_fwd_bwd(ptr(emb), ptr(dist), ptr(lab), ptr(demb), ptr(loss), ptr(coef), ptr(info), n, E, 0.2, 0, soft, stream()))
    torch.cuda.synchronize()
    assert info[0] > 0 and float(demb.abs().max()) > 0
    assert np.array_equal(_bits(got["loss"][:1]), _bits(loss[:1].cpu().numpy()))
    assert np.array_equal(_bits(got["coef"]), _bits(coef.cpu().numpy())) and np.array_equal(_bits(got["demb"]), _bits(demb.cpu().numpy()))
    assert np.array_equal(got["info"][:4], info[:4].cpu().numpy()) and not got["info"][4:].any()
    assert (got["mpick"] == -1).all() and not got["mcoef"].any()


# ---- 2. the smallest live case, the four sources of a pick -----------------------------------------------------------------------
@pytest.mark.parametrize("soft", [0, 1])
def test_smallest_live_case(lib, soft):
    """N = M = 2, labels [0, 1] on both sides: no in-batch positive, both rows are anchors only through the memory.  alpha = 10 is
    above every distance of rows of norm 1.5, so both hinges are active."""
    x, mem = _rows(2, 3, 2), _rows(2, 3, 3)
    got = _call(lib, x, [0, 1], mem, [0, 1], 2, 10.0, soft)
    _check(got, _oracle(got, x, [0, 1], mem, [0, 1], 2, 10.0, soft), soft, "N=M=2")
    assert list(got["info"][:5]) == [2, 2, 2, 0, 2] and got["info"][6] == 2 and list(got["mpick"][:, 0]) == [0, 1]
    assert (got["mcoef"][:, 0] > 0).all() and np.abs(got["demb"]).min(axis=1).max() > 0


FOUR_MPICK = [[0, -1], [0, 6], [-1, -1], [-1, 0], [2, 0], [4, 1]]     # worked out on the host; every pick is decided by more than 0.02


@pytest.mark.parametrize("soft", [0, 1])
def test_four_sources_of_a_pick(lib, soft):
    """N = 6, M = 7, E = 5: rows 2, 0, 3 and 1 take (p batch, n batch), (p memory, n batch), (p batch, n memory), (p memory, n memory);
    rows 4 and 5 have their only positives in the memory."""
    rng = np.random.default_rng(5)
    x, mem = rng.standard_normal((6, 5)).astype(np.float32), rng.standard_normal((7, 5)).astype(np.float32)
    labels, mlab = [0, 0, 1, 1, 2, 3], [0, 1, 2, 2, 3, 4, 5]
    got = _call(lib, x, labels, mem, mlab, 7, 0.2, soft)
    assert got["mpick"].tolist() == FOUR_MPICK
    assert list(got["info"]) == [6, 6, 6 if soft else 5, 0, 4, 4, 7, 0]
    _check(got, _oracle(got, x, labels, mem, mlab, 7, 0.2, soft), soft, "four sources")


# ---- 3. shapes -------------------------------------------------------------------------------------------------------------------
# N: below a wave, ragged, one wave, most of a workgroup; M: no multiple of 64 or 256, so the tails of the strided walk and of its
# four-fold unrolling are live, partly filled (M // 3) and full; E: 1, odd, the 512 limit, the production 128
SHAPES = [(3, 7, 1), (37, 300, 67), (64, 257, 512), (180, 1000, 128)]


def _shape_case(n, M, E):
    labels = bo.ragged_labels(n + M, seed=n + M + E)
    lab, mlab = labels[:n].copy(), labels[n:].copy()
    lab[-1], mlab[0], mlab[M // 3 - 1], mlab[-1] = 10 ** 6, -10 ** 6, lab[0], lab[0]     # one id only in the batch, one only in the memory
    return _rows(n, E, n * 1000 + E), lab, _rows(M, E, M * 1000 + E + 1), mlab


@pytest.mark.parametrize("soft", [0, 1])
@pytest.mark.parametrize("full", [False, True])
@pytest.mark.parametrize("n,M,E", SHAPES)
def test_shapes_partly_filled_and_full(lib, n, M, E, full, soft):
    x, lab, mem, mlab = _shape_case(n, M, E)
    valid = M if full else M // 3
    stale = mem.copy()
    stale[valid:] = np.nan                                             # (fn_pairwise_sqdist turns these into 0: a tempting nearest negative)
    got = _call(lib, x, lab, stale, mlab, valid, 0.2, soft)
    o = _oracle(got, x, lab, mem, mlab, valid, 0.2, soft)
    assert o["Z"] > 0 and o["info"][4] + o["info"][5] > 0 and o["info"][6] == valid
    _check(got, o, soft, f"N={n} M={M} E={E} valid={valid} soft={soft}")
    loss_only = _call(lib, x, lab, stale, mlab, valid, 0.2, soft, with_grad=False)      # demb = NULL
    for k in ("loss", "coef", "info", "mpick", "mcoef"):
        assert np.array_equal(_bits(loss_only[k]), _bits(got[k])), k


# ---- 4. stale slots, a valid NaN ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("soft", [0, 1])
def test_stale_slots_are_never_looked_at(lib, soft):
    n, M, E, valid = 9, 20, 16, 8
    x, mem = _rows(n, E, 4), _rows(M, E, 5)
    lab = np.array([0, 0, 0, 1, 1, 1, 2, 2, 2])
    mlab = np.concatenate([[0, 1, 2, 0, 1, 2, 3, 3], np.resize([0, 1, 2], M - valid)])     # every anchor's own label sits in the stale part

    def poke(dist, mdist):
        mdist[:, valid:] = float("nan")
    clean = _call(lib, x, lab, mem, mlab, valid, 0.2, soft)
    got = _call(lib, x, lab, mem, mlab, valid, 0.2, soft, poke=poke)
    assert got["info"][3] == 0 and np.isfinite(got["loss"][0]) and got["info"][6] == valid and got["mpick"].max() < valid
    for k in ("loss", "coef", "demb", "info", "mpick", "mcoef"):
        assert np.array_equal(_bits(got[k]), _bits(clean[k])), k
    _check(got, _oracle(got, x, lab, mem, mlab, valid, 0.2, soft), soft, "stale")


@pytest.mark.parametrize("soft", [0, 1])
def test_a_nan_in_a_valid_slot_makes_the_loss_nan(lib, soft):
    n, M, E, valid = 9, 20, 16, 8
    x, mem = _rows(n, E, 4), _rows(M, E, 5)
    lab, mlab = np.array([0, 0, 0, 1, 1, 1, 2, 2, 2]), np.resize([0, 1, 2, 3], M)

    def poke(dist, mdist):
        mdist[4, valid - 1] = float("nan")
    got = _call(lib, x, lab, mem, mlab, valid, 0.2, soft, poke=poke)
    assert got["info"][3] == 1 and np.isnan(got["loss"][0]) and got["info"][0] == n and got["info"][6] == valid


# ---- 5. ties and exact zeros on lattice rows -----------------------------------------------------------------------------------
def _lattice():
    from tests import pair_lattice as pl
    sizes = [5, 4, 6, 3]
    x, _, H = pl.lattice_classes(sizes, seed=3, flips=8)
    return x, np.repeat(np.arange(len(sizes)), sizes), H


@pytest.mark.parametrize("soft", [0, 1])
def test_a_batch_row_beats_a_memory_slot_at_the_same_distance(lib, soft):
    """The memory is a copy of the batch under the same labels: every candidate has a twin at bitwise the same distance, the batch
    column the lower union index.  (An anchor's own copy is a positive at distance 0 and never the farthest.)"""
    x, lab, H = _lattice()
    n = len(lab)
    got = _call(lib, x, lab, x, lab, n, 1.0, soft)
    assert np.array_equal(got["dist"], (H / 16.0).astype(np.float32)) and np.array_equal(got["mem_dist"], got["dist"])
    assert (got["mpick"] == -1).all() and not got["mcoef"].any() and not got["info"][4:6].any() and got["info"][0] == n
    _check(got, _oracle(got, x, lab, x, lab, n, 1.0, soft), soft, "batch wins")
    batch_only = bo.mine(got["dist"], lab, 1.0, 0, soft)
    assert np.array_equal(got["coef"] != 0, batch_only["coef"] != 0)


@pytest.mark.parametrize("soft", [0, 1])
def test_the_lower_of_two_slots_at_the_same_distance_wins(lib, soft):
    """The batch is the first row of every class, the memory all rows twice: an anchor's positives sit only in the memory and each
    has a twin n slots higher."""
    x, lab, H = _lattice()
    n = len(lab)
    first = np.flatnonzero(np.r_[True, lab[1:] != lab[:-1]])
    mem, mlab = np.concatenate([x, x]), np.concatenate([lab, lab])
    got = _call(lib, x[first], lab[first], mem, mlab, 2 * n, 1.0, soft)
    assert np.array_equal(got["mem_dist"][:, :n], got["mem_dist"][:, n:])
    assert got["info"][0] == len(first) == got["info"][4] and (got["mpick"][:, 0] >= 0).all() and got["mpick"].max() < n
    _check(got, _oracle(got, x[first], lab[first], mem, mlab, 2 * n, 1.0, soft), soft, "lower slot wins")


def test_an_exact_zero_hinge_with_a_memory_pick_is_an_inactive_term(lib):
    """Sign rows of amplitude 1/8 in 64 columns: d = h / 16.  Anchor A: its only positive is slot 0 at h = 8 (d = 0.5), its nearest
    negative the batch row B at h = 24 (d = 1.5); with alpha = 1 the hinge is exactly 0: a term, inactive, mcoef 0.  Anchor B: positive
    slot 1 at d = 1, negative A: hinge 0.5, active."""
    S = np.ones((4, 64))
    S[1, :24] = -1                                                     # B
    S[2, 56:] = -1                                                     # P: label 0
    S[3] = S[1]
    S[3, 24:40] *= -1                                                  # Q: label 1
    rows = (S / 8).astype(np.float32)
    mem = np.concatenate([rows[2:], np.full((1, 64), np.nan, np.float32)])
    got = _call(lib, rows[:2], [0, 1], mem, [0, 1, 0], 2, 1.0, 0)
    assert got["dist"][0, 1] == 1.5 and got["mem_dist"][:, :2].tolist() == [[0.5, 2.5], [2.0, 1.0]]
    assert list(got["info"]) == [2, 2, 1, 0, 2, 0, 2, 0]
    assert got["mpick"].tolist() == [[0, -1], [1, -1]] and got["mcoef"].tolist() == [[0.0, 0.0], [1.0, 0.0]]
    assert got["coef"].tolist() == [[0.0, 0.0], [-1.0, 0.0]] and got["loss"][0] == 0.25
    _check(got, _oracle(got, rows[:2], [0, 1], mem, [0, 1, 0], 2, 1.0, 0), 0, "exact zero")


# ---- 6. the ring -----------------------------------------------------------------------------------------------------------------
def _enqueue(lib, emb, labels, mem, mlab, state, start):
    n, E = emb.shape
    _lib.check(lib.fn_xbm_enqueue(ptr(emb), ptr(labels), ptr(mem), ptr(mlab), ptr(state), n, mem.shape[0], E, start, stream()))
    torch.cuda.synchronize()


def test_ring_follows_the_host_model(lib):
    M, n, E = 7, 3, 5
    model = xo.Ring(M, E)
    mem = torch.full((M * E + TAIL,), POISON, device="cuda")
    mlab = torch.full((M + TAIL,), 77, dtype=torch.int32, device="cuda")
    state = torch.zeros(4 + TAIL, dtype=torch.int32, device="cuda")
    state[4:] = 77
    model.emb[:], model.labels[:] = POISON, 77
    for call in range(5):                                              # start = 2: two counted calls, then slots 0-2, 3-5 and 6, 0, 1
        emb, labels = _rows(n, E, 40 + call), np.arange(n) + 10 * call
        _enqueue(lib, _dev(emb, np.float32), _dev(labels, np.int32), mem[:M * E].view(M, E), mlab, state, 2)
        model.enqueue(emb, labels, start=2)
        assert state[:4].cpu().tolist() == model.state.tolist()
        assert np.array_equal(_bits(mem[:M * E].view(M, E).cpu().numpy()), _bits(model.emb)) and np.array_equal(mlab[:M].cpu().numpy(), model.labels)
        assert bool((mem[M * E:] == POISON).all()) and bool((mlab[M:] == 77).all()) and bool((state[4:] == 77).all())
    assert model.state.tolist() == [2, 7, 5, 0]


def test_ring_whole_memory_batches_and_refusals(lib):
    M = E = 3
    model = xo.Ring(M, E)
    mem, mlab, state = torch.zeros(M, E, device="cuda"), torch.zeros(M, dtype=torch.int32, device="cuda"), torch.zeros(4, dtype=torch.int32, device="cuda")
    for call in range(2):                                              # N = M: every call overwrites everything
        emb, labels = _rows(M, E, 50 + call), np.arange(M) + 10 * call
        _enqueue(lib, _dev(emb, np.float32), _dev(labels, np.int32), mem, mlab, state, 0)
        model.enqueue(emb, labels)
        assert state.cpu().tolist() == model.state.tolist() == [0, 3, call + 1, 0]
        assert np.array_equal(_bits(mem.cpu().numpy()), _bits(emb)) and mlab.cpu().tolist() == labels.tolist()
    big, lab = torch.zeros(1100, 4, device="cuda"), torch.zeros(1100, dtype=torch.int32, device="cuda")
    before = (mem.clone(), mlab.clone(), state.clone())

    def call(n=2, M=M, E=E, start=0, null=None):
        a = [ptr(big), ptr(lab), ptr(mem), ptr(mlab), ptr(state)]
        if null is not None:
            a[null] = None
        _lib.check(lib.fn_xbm_enqueue(*a, n, M, E, start, stream()))
    for kw in (dict(n=4), dict(n=0), dict(n=1025, M=2000), dict(M=65537), dict(E=0), dict(E=513), dict(start=-1), *(dict(null=i) for i in range(5))):
        with pytest.raises(ValueError):                                # N > M among them
            call(**kw)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, (mem, mlab, state)))


# ---- 7. reproducibility, refusals, the wrapper -----------------------------------------------------------------------------------
@pytest.mark.parametrize("soft", [0, 1])
def test_same_call_same_bits(lib, soft):
    x, lab, mem, mlab = _shape_case(180, 1000, 128)
    a, b = (_call(lib, x, lab, mem, mlab, 1000, 0.2, soft) for _ in range(2))
    for k in ("loss", "coef", "demb", "info", "mpick", "mcoef"):
        assert np.array_equal(_bits(a[k]), _bits(b[k])), k


def test_limits_and_bad_settings_are_refused(lib):
    names = ["emb", "dist", "labels", "mem_emb", "mem_dist", "mem_labels", "mem_state", "demb", "loss", "coef", "mpick", "mcoef", "info"]
    ints = {"labels", "mem_labels", "mem_state", "mpick", "info"}
    bufs = {k: torch.zeros(4096, dtype=torch.int32 if k in ints else torch.float32, device="cuda") for k in names}

    def call(n=4, M=8, E=8, alpha=0.2, soft=0, null=None, loss_off=0):
        a = {k: ptr(t) for k, t in bufs.items()}
        a["loss"] = ptr(bufs["loss"], loss_off)
        if null:
            a[null] = None
        _lib.check(lib.fn_xbm_triplet_fwd_bwd(*(a[k] for k in names), n, M, E, alpha, soft, stream()))
    call()
    call(alpha=-1.0, soft=1)                                           # alpha is ignored under a soft margin
    call(null="demb")
    call(n=8, M=8)
    torch.cuda.synchronize()
    for t in bufs.values():
        t.fill_(3)
    bad = [dict(n=1025, M=2000), dict(n=1), dict(n=9, M=8), dict(M=3), dict(M=65537), dict(E=513), dict(E=0), dict(alpha=-0.1),
           dict(alpha=float("nan")), dict(alpha=float("inf")), dict(soft=2), dict(soft=-1), dict(loss_off=1)]
    for kw in bad + [dict(null=k) for k in names if k != "demb"]:
        with pytest.raises(ValueError):
            call(**kw)
    torch.cuda.synchronize()
    assert all(bool((t == 3).all()) for t in bufs.values())           # a refusal launches nothing


def test_wrapper_owns_the_ring(lib):
    from facenet_amd.triplet import CrossBatchMemory
    n, E, M = 12, 16, 30
    memory = CrossBatchMemory(M, E, "cuda")
    assert memory.valid == 0 and tuple(memory.emb.shape) == (M, E)
    x1, x2 = _rows(n, E, 60, scale=3.0), _rows(n, E, 61, scale=0.5)
    l1, l2 = np.repeat([4, 9, -3, 70], 3), np.repeat([9, 4, 70, 8], 3)
    memory.enqueue(torch.from_numpy(x1), l1)
    assert memory.valid == n and memory.state.cpu().tolist() == [n, n, 1, 0] and memory.labels[:n].cpu().tolist() == l1.tolist()
    np.testing.assert_allclose(memory.emb[:n].cpu().numpy(), x1 / 3.0, rtol=0, atol=1e-6)      # the ring holds normalised rows
    loss, grad, info, picks = memory.loss(torch.from_numpy(x2).cuda(), l2, alpha=0.3)
    assert memory.state.cpu().tolist() == [n, n, 1, 0]                # the loss does not enqueue
    e2 = _dev(x2, np.float32)
    embn, want = torch.empty_like(e2), torch.empty_like(e2)
    _lib.check(lib.fn_l2norm_fwd(ptr(e2), ptr(embn), n, E, 1e-10, stream()))
    got = _call(lib, embn.cpu().numpy(), l2, memory.emb.cpu().numpy(), memory.labels.cpu().numpy(), n, 0.3, 0)
    dembn = _dev(got["demb"], np.float32)
    _lib.check(lib.fn_l2norm_bwd(ptr(e2), ptr(dembn), ptr(want), n, E, 1e-10, stream()))
    assert float(loss) == got["loss"][0] and torch.equal(grad, want) and np.array_equal(picks.cpu().numpy(), got["mpick"])
    assert [info["anchors"], info["terms"], info["active"], info["memory_positives"], info["memory_negatives"], info["memory_valid"]] == \
        [int(got["info"][i]) for i in (0, 1, 2, 4, 5, 6)] and info["memory_valid"] == n and info["memory_positives"] > 0
    memory.reset()
    assert memory.valid == 0 and not memory.state.any()
    for bad in (lambda: CrossBatchMemory(1, E), lambda: CrossBatchMemory(65537, E), lambda: CrossBatchMemory(M, 513),
                lambda: memory.enqueue(torch.zeros(M + 1, E), np.zeros(M + 1)), lambda: memory.loss(torch.zeros(n, E + 1), l2),
                lambda: memory.loss(torch.zeros(n, E), l2[:5])):
        with pytest.raises(ValueError):
            bad()


# ---- 8. the Trainer --------------------------------------------------------------------------------------------------------------
HEAD_OPS = ["l2norm_fwd", "pairwise_sqdist", "pairwise_sqdist", "xbm_triplet", "l2norm_bwd", "xbm_enqueue"]
P_, K_, M_ = 4, 3, 30                                                  # batch 12 in a ring of 30: the third step's rows wrap
N_ = P_ * K_
IDS = np.array([11, -4, 7, 300, 52, 8])                                # dataset-wide identity ids; a step sees four of them


def _net(seed=0):
    return Network(embedding_size=128, device="cuda:0", train_dtype=torch.float16, seed=seed)


def _label_sets(steps, seed):
    rng = np.random.default_rng(seed)
    return [rng.permutation(np.repeat(rng.permutation(IDS)[:P_], K_)) for _ in range(steps)]


def _trainer(params, seed=3, soft=False, **kw):
    net = _net(seed)
    net.load_keras_params(params)
    kw.setdefault("memory_size", M_)
    return Trainer(net, batch=N_, loss="triplet", lr=0.01, triplet_strategy="batch_hard", soft_margin=soft, **kw)


def _ring(tr):
    return [t.cpu().numpy().copy() for t in (tr.mem_emb, tr.mem_labels, tr.mem_state)]


def _run_steps(params, x, graph, steps=3, **kw):
    tr = _trainer(params, **kw)
    labels = _label_sets(steps, 6)
    tr.set_images(x, labels[0])
    if graph:
        before = _ring(tr)
        tr.capture()
        torch.cuda.synchronize()
        assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(before, _ring(tr)))      # capture() leaves the memory as it found it
    out = []
    for s in range(steps):
        tr.set_images(x, labels[s])
        tr.step()
        torch.cuda.synchronize()
        out += [tr.emb.cpu().numpy().copy(), tr.coef.cpu().numpy().copy(), tr.mpick.cpu().numpy().copy(), tr.mcoef.cpu().numpy().copy(),
                tr.loss.cpu().numpy()[:1].copy(), tr.mine_info.cpu().numpy().copy()] + _ring(tr)
    assert np.isfinite(tr.loss_value())
    return out + [tr.net.P.cpu().numpy()], tr


@pytest.fixture(scope="module")
def params():
    return _net().export_keras_params()


@pytest.mark.parametrize("soft", [False, True])
def test_step_stage_by_stage(params, soft):
    """The second step of a run, so that the memory holds the first step's rows: every stage against its oracle."""
    tr = _trainer(params, soft=soft)
    assert [op.name for op in tr.loss_ops] == HEAD_OPS and tr.head.state == ("mem_emb", "mem_labels", "mem_state")
    labels = _label_sets(2, 2)
    x = torch.from_numpy(structured_images(N_, seed=21))
    tr.set_images(x, labels[0])
    tr.step()
    torch.cuda.synchronize()
    assert tr.mem_state.cpu().tolist() == [N_, N_, 1, 0] and tr.mem_labels[:N_].cpu().tolist() == labels[0].tolist()
    assert torch.equal(tr.mem_emb[:N_], tr.embn) and tr.triplet_stats()["memory_valid"] == 0
    mem, mlab, _ = _ring(tr)
    tr.set_images(x, labels[1])
    st = tr.net.stream()
    tr._zero()
    for ops in (tr.plan.fwd, tr.loss_ops, tr.plan.bwd):
        tr.plan.run_ops(ops, st)
    torch.cuda.synchronize()
    emb, embn = tr.emb.cpu(), tr.embn.cpu()
    ref, bound, _, _ = eo.l2norm_ref(emb, 1e-10)
    eo.check_bound(embn, ref, bound, "embn")
    got = dict(dist=tr.dist.cpu().numpy(), mem_dist=tr.mem_dist.cpu().numpy(), info=tr.mine_info.cpu().numpy(), coef=tr.coef.cpu().numpy(),
               loss=tr.loss.cpu().numpy(), demb=tr.dembn.cpu().numpy(), mpick=tr.mpick.cpu().numpy(), mcoef=tr.mcoef.cpu().numpy())
    assert np.array_equal(got["dist"], fo.squared_distance_matrix(embn.numpy()))
    o = xo.mine(got["dist"], got["mem_dist"], labels[1], mlab, N_, 0.2, int(soft), emb=embn.numpy(), mem=mem)
    assert o["info"][0] == N_ and o["info"][4] + o["info"][5] > 0
    _check(got, o, int(soft), f"trainer soft={soft}")
    stats = tr.triplet_stats()
    assert [stats["anchors"], stats["active"], stats["memory_valid"], stats["memory_positives"], stats["memory_negatives"]] == \
        [int(o["info"][i]) for i in (0, 2, 6, 4, 5)]
    ref, bound, ok = eo.l2norm_bwd_ref(emb, tr.dembn.cpu(), 1e-10)
    assert ok
    eo.check_bound(tr.demb.cpu(), ref, bound, "demb")
    assert float(tr.G.abs().max()) > 0 and bool(torch.isfinite(tr.G).all())
    # the enqueue came last: the first step's rows are untouched, this step's rows follow them
    assert torch.equal(tr.mem_emb[:N_].cpu(), torch.from_numpy(mem[:N_])) and torch.equal(tr.mem_emb[N_:2 * N_], tr.embn)
    assert tr.mem_state.cpu().tolist() == [2 * N_, 2 * N_, 2, 0] and tr.mem_labels[N_:2 * N_].cpu().tolist() == labels[1].tolist()
    tr.reset_memory()
    assert not tr.mem_state.any()


def test_three_steps_eager_and_captured_are_bitwise_equal(params):
    x = torch.from_numpy(structured_images(N_, seed=22))
    eager, tr = _run_steps(params, x, graph=False)
    assert tr.mem_state.cpu().tolist() == [3 * N_ - M_, M_, 3, 0]       # the ring wrapped inside the third step
    assert eager[5][6] == 0 and eager[14][6] == N_ and eager[23][6] == 2 * N_ and eager[23][4] + eager[23][5] > 0
    captured, _ = _run_steps(params, x, graph=True)
    for a, b in zip(eager, captured):
        assert np.array_equal(_bits(a), _bits(b))


def test_memory_start_delays_the_first_enqueue(params):
    x = torch.from_numpy(structured_images(N_, seed=22))
    out, tr = _run_steps(params, x, graph=True, memory_start=2)
    assert [out[9 * s + 8].tolist() for s in range(3)] == [[0, 0, 1, 0], [0, 0, 2, 0], [N_, N_, 3, 0]]
    assert [int(out[9 * s + 5][6]) for s in range(3)] == [0, 0, 0] and not any(out[9 * s + 2].max() >= 0 for s in range(3))
    assert torch.equal(tr.mem_emb[:N_], tr.embn)


def test_memory_less_trainer_is_untouched_by_a_memory_in_the_process(params):
    x = torch.from_numpy(structured_images(N_, seed=23))
    labels = np.repeat(IDS[:P_], K_)

    def plain(**kw):
        net = _net(seed=1)
        net.load_keras_params(params)
        tr = Trainer(net, batch=N_, loss="triplet", lr=0.01, triplet_strategy="batch_hard", **kw)
        tr.set_images(x, labels)
        for _ in range(2):
            tr.step()
        torch.cuda.synchronize()
        return tr
    a = plain()
    _run_steps(params, x, graph=False, steps=1)
    b = plain(memory_size=0, memory_start=0)
    names = [op.name for op in b.step_ops]
    assert [op.name for op in a.step_ops] == names and "batch_triplet" in names and "xbm_enqueue" not in names
    assert not hasattr(b, "mem_emb") and sorted(b.triplet_stats()) == ["active", "active_fraction", "anchors", "terms"]
    assert torch.equal(a.G, b.G) and torch.equal(a.net.P, b.net.P) and torch.equal(a.loss[:1], b.loss[:1]) and float(a.G.abs().max()) > 0
    with pytest.raises(RuntimeError, match="no cross-batch memory"):
        b.reset_memory()


def test_checkpoint_round_trip(params, tmp_path):
    x = torch.from_numpy(structured_images(N_, seed=24))
    labels = _label_sets(3, 8)

    def trainer(seed, **kw):
        tr = _trainer(params, seed=seed, **kw)
        tr.set_images(x, labels[0])
        return tr
    tr = trainer(0)
    tr.step()
    tr.set_images(x, labels[1])
    tr.step()
    path = tmp_path / "ckpt.npz"
    tr.save_checkpoint(path, epoch=1)
    tr.set_images(x, labels[2])
    tr.step()
    torch.cuda.synchronize()
    with np.load(path) as z:
        assert {"xbm/embeddings:0", "xbm/labels:0", "xbm/state:0"} <= set(z.files) and z["xbm/state:0"].tolist() == [2 * N_, 2 * N_, 2, 0]
    tr2 = trainer(5)
    assert tr2.load_checkpoint(path) == 1
    tr2.set_images(x, labels[2])
    tr2.step()
    torch.cuda.synchronize()
    a, b = tr.net.export_keras_params(), tr2.net.export_keras_params()
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert torch.equal(tr.loss[:1], tr2.loss[:1]) and torch.equal(tr.mpick, tr2.mpick) and tr2.triplet_stats()["memory_valid"] == 2 * N_
    assert all(np.array_equal(_bits(p), _bits(q)) for p, q in zip(_ring(tr), _ring(tr2)))
    # another M, or a checkpoint without a memory: an empty memory and a warning
    other = trainer(5, memory_size=N_)
    other.step()
    with pytest.warns(UserWarning, match="holds a memory of 30 x 128"):
        other.load_checkpoint(path)
    assert not other.mem_state.any()
    plain = Trainer(_net(1), batch=N_, loss="triplet", lr=0.01, triplet_strategy="batch_hard")
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        plain.load_checkpoint(path)                                    # a memory-less trainer reads the checkpoint without a word
    plain.save_checkpoint(tmp_path / "plain.npz")
    tr2.step()
    with pytest.warns(UserWarning, match="holds no cross-batch memory"):
        tr2.load_checkpoint(tmp_path / "plain.npz")
    assert not tr2.mem_state.any()


# ---- 9. the one-rank process group ---------------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _one_rank(port, q):
    import torch.distributed as dist
    os.environ["FACENET_AUTOTUNE"] = "0"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1, device_id=dev)
    try:
        params, _, _ = fo.build_params(128, seed=0)
        x = torch.from_numpy(structured_images(N_, seed=25))
        out, tr = _run_steps(params, x, graph=False, steps=2, world_size=1, process_group=dist.group.WORLD, n_buckets=4)
        assert tr.exchange and len(tr.segments) == len(tr.buckets) + 1
        q.put((out[-1], tr.G.cpu().numpy(), tr.loss_value(), _ring(tr)))
    finally:
        dist.destroy_process_group()


def test_one_rank_process_group_equals_the_plain_step():
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_one_rank, args=(_free_port(), q))
    p.start()
    try:
        P, G, loss, ring = q.get(timeout=600)
        p.join(timeout=120)
        assert p.exitcode == 0
    finally:
        if p.is_alive():
            p.kill()
    params, _, _ = fo.build_params(128, seed=0)
    x = torch.from_numpy(structured_images(N_, seed=25))
    out, tr = _run_steps(params, x, graph=False, steps=2)
    assert float(np.abs(G).max()) > 0 and tr.mem_state.cpu().tolist() == [2 * N_, 2 * N_, 2, 0]
    assert np.array_equal(G, tr.G.cpu().numpy()) and np.array_equal(P, out[-1]) and loss == tr.loss_value()
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(ring, _ring(tr)))


# ---- 10. the app -------------------------------------------------------------------------------------------------------------------
def test_app_runs_an_epoch_logs_the_memory_share_and_refuses_unlabelled_pools():
    from facenet_amd.apps.train_tripletloss import train_tripletloss
    from facenet_amd.config import load_config
    logs = []
    cfg = load_config(overrides={"loss": {"triplet_strategy": "batch_hard", "memory_size": M_},
                                 "train": {"epoch": {"nrof_epochs": 1, "size": 3}, "learning_rate": {"value": 0.01}}})
    x = torch.from_numpy(structured_images(N_, seed=26))
    labels = _label_sets(3, 9)
    net, tr = train_tripletloss(cfg, people_per_batch=P_, images_per_person=K_, pools=iter([(x, lab) for lab in labels]), log=logs.append)
    assert logs[0] == f"triplet strategy: batch_hard, cross-batch memory: {M_} rows from step 0" and len(logs) == 2
    assert tr.memory_size == M_ and tr._graph is not None and [op.name for op in tr.loss_ops] == HEAD_OPS
    assert tr.mem_state.cpu().tolist() == [3 * N_ - M_, M_, 3, 0]       # capture()'s warm-up step left no trace
    stats = tr.triplet_stats()
    assert stats["memory_valid"] == 2 * N_ and stats["anchors"] == N_
    share = float(logs[1].split("memory negatives ")[1].split()[0])
    assert abs(share - stats["memory_negatives"] / N_) <= 5e-4 and f"({2 * N_} rows)" in logs[1]
    assert np.isfinite(float(logs[1].split("triplet loss ")[1].split()[0]))
    with pytest.raises(ValueError, match="pools must yield \\(images, labels\\)"):
        train_tripletloss(cfg, people_per_batch=P_, images_per_person=K_, pools=iter([x]), use_graph=False, log=logs.append)
