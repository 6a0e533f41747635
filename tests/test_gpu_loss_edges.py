"""The kernels of csrc/loss.hip at their edge shapes: softmax cross-entropy, triplet loss, the distance matrix and the online
triplet selection.  Losses and gradients are bounded element by element against fp64 (tests/elementwise_oracle.py); the distance
matrix and the selected triplets are compared bit for bit with the oracle, which selects on the matrix the device produced."""
import numpy as np
import pytest
import torch

from facenet_amd import _lib
from oracle import facenet_oracle as fo
from tests import elementwise_oracle as eo
from tests.util import ACC_GRAD_BITS, bitpattern, gamma, lp_dtype, ptr, same_bits, stream

pytestmark = pytest.mark.gpu
BF, HF = _lib.FN_BF16, _lib.FN_F16
JUNK = 0x5A5A5A5A5A5A


# ---- softmax cross-entropy ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [BF, HF])
@pytest.mark.parametrize("N,C,ld,ld_d", [(6, 37, 40, 40),            # one trip, three waves contribute only their identity
                                         (90, 1000, 1000, 1008),    # four trips, the last one partial; ld_d > C with ld == C
                                         (7, 8631, 8640, 8632)])    # production class count, ld > C and ld_d > C, ld != ld_d
def test_softmax_xent_edges(lib, N, C, ld, ld_d, dt):
    """Logits at scale 3 with a per-row offset of +-80, labels in column 0 and C - 1, logits' padding columns poisoned, dlogits'
    padding columns zero up to ld_d and untouched beyond, dlogits = NULL, dbias = NULL."""
    x, labels = eo.softmax_inputs(N, C, ld, seed=N)
    ref = eo.softmax_ref(x, labels, C, 1.0 / N)
    xd, ld_dev = x.cuda(), labels.cuda()
    e_lp = ref["e_g"] + eo.U_LP[dt] * (ref["g"].abs() + ref["e_g"]) + eo.ETA_LP[dt]
    for with_dl, with_db in ((True, True), (True, False), (False, False)):
        loss = torch.full((4,), 7.0, device="cuda")
        dl = bitpattern((N * ld_d + 16,), dt)
        before = dl.clone()
        dbias = torch.zeros(C + 8, dtype=torch.int64, device="cuda")
        dbias[C:] = JUNK
        _lib.check(lib.fn_softmax_xent_fwd_bwd(ptr(xd), ld, ptr(ld_dev), ptr(loss), ptr(dl) if with_dl else None, ld_d, ptr(dbias) if with_db else None,
                                               N, C, 1.0 / N, dt, stream()))
        torch.cuda.synchronize()
        eo.check_bound(loss[0], ref["loss"], ref["e_loss"], "softmax loss")
        if with_dl:
            got = dl[:N * ld_d].view(N, ld_d).cpu()
            eo.check_bound(got[:, :C], ref["g"], e_lp, "dlogits")
            assert float(got[:, C:].float().abs().max()) == 0, "padding columns of dlogits"
            assert same_bits(dl[N * ld_d:], before[N * ld_d:])
        else:
            assert same_bits(dl, before)
        if with_db:
            eo.check_bound(dbias[:C].cpu().double() * 2.0 ** -ACC_GRAD_BITS, ref["dbias"], ref["e_dbias"], "dbias")
        else:
            assert int(dbias[:C].abs().max()) == 0
        assert bool((dbias[C:] == JUNK).all())


# ---- triplet loss -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha", [0.2, 0.0])
@pytest.mark.parametrize("T,E", [(1, 128), (7, 128), (30, 512), (5, 8)])      # E = 512: 8 trips per lane; E = 8: 56 idle lanes; T = 1
def test_triplet_loss_edges(lib, T, E, alpha):
    """Clearly active and clearly inactive triplets; the last triplet has p == n bit for bit: with alpha = 0 its hinge is exactly 0
    and its three gradient rows are exactly 0."""
    emb = eo.triplet_inputs(T, E, alpha, seed=T)
    ref = eo.triplet_ref(emb, T, E, alpha)
    clear = (ref["l"].abs() > ref["e_l"]) | (ref["same"] & (alpha == 0.0))
    assert bool(clear.all()), "a hinge whose sign is ambiguous in fp32"                 # share of excluded triplets: 0
    ed = emb.cuda()
    demb = torch.full((3 * T + 1, E), 7.0, device="cuda")
    loss = torch.full((4,), 7.0, device="cuda")
    _lib.check(lib.fn_triplet_loss_fwd_bwd(ptr(ed), ptr(demb), ptr(loss), T, E, alpha, stream()))
    torch.cuda.synchronize()
    eo.check_bound(loss[0], ref["loss"], ref["e_loss"], "triplet loss")
    eo.check_bound(demb[:3 * T], ref["grad"], ref["e_grad"], "triplet gradient")
    assert float(demb[3 * T].min()) == 7.0 and float(demb[3 * T].max()) == 7.0
    if alpha == 0.0:
        assert float(demb[3 * (T - 1):3 * T].abs().max()) == 0
    loss2 = torch.full((4,), 7.0, device="cuda")
    _lib.check(lib.fn_triplet_loss_fwd_bwd(ptr(ed), None, ptr(loss2), T, E, alpha, stream()))      # demb = NULL: the loss alone
    torch.cuda.synchronize()
    assert torch.equal(loss2[:1], loss[:1])


# ---- distance matrix ----------------------------------------------------------------------------------------------------
def _embeddings(P, K, E, seed, noise=0.08, spread=0.05):
    rng = np.random.default_rng(seed)
    emb = rng.normal(size=(P * K, E)).astype(np.float32) * noise + rng.normal(size=(P, 1, E)).astype(np.float32).repeat(K, 1).reshape(P * K, E) * spread
    return emb / np.linalg.norm(emb, axis=1, keepdims=True)


@pytest.mark.parametrize("n,E", [(48, 64), (180, 128), (180, 512), (70, 72)])     # fma chains of 1, 2, 8; E = 72: a ragged second register
def test_pairwise_sqdist_bits_and_symmetry(lib, n, E):
    from facenet_amd.triplet import squared_distances
    emb = _embeddings(n // 2, 2, E, seed=E)[:n]
    dist = squared_distances(torch.from_numpy(emb).cuda()).cpu().numpy()
    assert np.array_equal(dist, dist.T), "the distance matrix is not bitwise symmetric"
    assert np.array_equal(dist, fo.squared_distance_matrix(emb))


@pytest.mark.parametrize("metric", [0, 1])
def test_pairwise_similarities_rectangular(lib, metric):
    """n != m, m > 64 (a second blockIdx.x), E = 72; every element bounded: the dot product is a chain of 2 fused multiply-adds
    and 6 butterfly adds (gamma_8 over sum |a||b|), metric 0 adds fl(1 - s) and the doubling (exact), metric 1 acosf (slack of 4
    ulps by the rule of the other device functions, and the argument error times 1 / sqrt(1 - s^2)); `range` against the fp64
    minimum / maximum of the dot products."""
    n, m, E = 23, 150, 72
    rng = np.random.default_rng(3)
    xa = rng.normal(size=(n, E)).astype(np.float32)
    xa /= np.linalg.norm(xa, axis=1, keepdims=True)
    xb = rng.normal(size=(m, E)).astype(np.float32)
    xb /= np.linalg.norm(xb, axis=1, keepdims=True)
    a, b = torch.from_numpy(xa).cuda(), torch.from_numpy(xb).cuda()
    out = torch.full((n * m + 4,), 7.0, device="cuda")
    rng_words = torch.zeros(2, dtype=torch.int32, device="cuda")
    _lib.check(lib.fn_pairwise_sqdist(ptr(a), ptr(b), ptr(out), ptr(rng_words), n, m, E, metric, stream()))
    torch.cuda.synchronize()
    d = torch.from_numpy(xa).double() @ torch.from_numpy(xb).double().T
    e_d = gamma(8) * (torch.from_numpy(xa).double().abs() @ torch.from_numpy(xb).double().abs().T)
    assert float(d.abs().max() + e_d.max()) < 0.9            # the clip to [-1, 1] is inactive and acos is well conditioned
    if metric == 0:
        ref, bound = 2 * (1 - d), 2 * e_d + 2 * eo.U * ((1 - d).abs() + e_d)
    else:
        ref = torch.acos(d)
        bound = e_d / (1 - (d.abs() + e_d) ** 2).sqrt() + 2 * 4 * eo.U * ref.abs()
    eo.check_bound(out[:n * m].view(n, m), ref, bound, f"metric {metric}")
    assert float(out[n * m:].min()) == 7.0 and float(out[n * m:].max()) == 7.0
    v = rng_words.cpu().numpy()
    lo, hi = np.where(v >= 0, v, v ^ 0x7fffffff).astype(np.int32).view(np.float32)
    assert abs(float(lo) - float(d.min())) <= float(e_d.max()) and abs(float(hi) - float(d.max())) <= float(e_d.max())


# ---- online triplet selection ---------------------------------------------------------------------------------------------
def _select_case(labels, emb, T, alpha=0.2, seeds=(0, 123)):
    from facenet_amd.triplet import select_triplets, squared_distances
    dist = squared_distances(torch.from_numpy(emb).cuda())
    dnp = dist.cpu().numpy()
    assert np.array_equal(dnp, dnp.T)
    infos = []
    for semi in (False, True):
        for seed in seeds:
            trip, info = select_triplets(dist, labels, alpha, T, seed=seed, semi_hard=semi)
            ref = fo.select_triplets(dnp, labels, alpha, T, seed, semi_hard=semi)
            assert np.array_equal(trip.cpu().numpy(), ref), (semi, seed)
            infos.append(info)
    _, counts = np.unique(labels, return_counts=True)
    assert all(i["pairs"] == int((counts * (counts - 1) // 2).sum()) for i in infos)
    return dist, infos


def test_select_triplets_production_pool(lib):
    """45 x 4 (n = 180): the cross-wave carry of the prefix scan, the second and third j0 trips and the want -= cnt carry."""
    labels = np.repeat(np.arange(45), 4)
    _, infos = _select_case(labels, _embeddings(45, 4, 128, seed=1), T=200)
    assert all(i["valid"] > 0 for i in infos)                 # the candidate pick (not only the fallback) ran


def test_select_triplets_past_the_lds_stage(lib):
    """10 x 32 (n = 320): 4960 pairs, 864 of them ranked by the remainder loop beyond the 4096 staged keys."""
    labels = np.repeat(np.arange(10), 32)
    _select_case(labels, _embeddings(10, 32, 128, seed=2), T=4500, seeds=(0,))
    _select_case(labels, _embeddings(10, 32, 128, seed=2), T=1000, seeds=(123,))


def test_select_triplets_unequal_classes_and_a_singleton(lib):
    sizes = [1, 2, 5, 9, 17, 40]                               # n = 74: class 0 has one image and contributes no pair
    labels = np.repeat(np.arange(len(sizes)), sizes)
    rng = np.random.default_rng(4)
    perm = rng.permutation(len(labels))                        # classes interleaved: pair ids are not grouped by class
    emb = _embeddings(len(sizes), 40, 64, seed=4)
    emb = np.concatenate([emb[40 * c:40 * c + s] for c, s in enumerate(sizes)])
    _select_case(labels[perm], emb[perm], T=300)


def test_select_triplets_pairs_without_a_candidate_are_topped_up(lib):
    """Tight, well separated identities next to overlapping ones: some pairs have no negative within the margin (cls = 1) and are
    taken, in key order, only after every pair with a candidate; T = all pairs, so the fallback class is used."""
    P, K, E = 20, 4, 64
    emb = _embeddings(P, K, E, seed=5)
    tight = _embeddings(P, K, E, seed=6, noise=0.002, spread=1.0)
    emb[:P * K // 2] = tight[:P * K // 2]
    labels = np.repeat(np.arange(P), K)
    pairs = P * K * (K - 1) // 2
    _, infos = _select_case(labels, emb, T=pairs)
    assert all(0 < i["valid"] < i["pairs"] for i in infos), infos      # the fallback class was actually used


def test_select_triplets_call_counter_advances_the_seed(lib):
    """Two calls on one info buffer: the second equals the oracle at seed + 1 (a replayed graph draws fresh negatives)."""
    from facenet_amd.triplet import squared_distances
    labels = np.repeat(np.arange(45), 4)
    emb = _embeddings(45, 4, 128, seed=1)
    dist = squared_distances(torch.from_numpy(emb).cuda())
    n, T, seed = 180, 200, 40
    lab = torch.from_numpy(labels.astype(np.int32)).cuda()
    info = torch.zeros(8 + 5 * (n * (n - 1) // 2), dtype=torch.int32, device="cuda")
    for call in range(2):
        trip = torch.full((T + 1, 3), -7, dtype=torch.int32, device="cuda")
        _lib.check(lib.fn_select_triplets(ptr(dist), ptr(lab), n, 0.2, T, seed, 0, ptr(trip), ptr(info), stream()))
        torch.cuda.synchronize()
        assert np.array_equal(trip[:T].cpu().numpy(), fo.select_triplets(dist.cpu().numpy(), labels, 0.2, T, seed + call))
        assert bool((trip[T] == -7).all()) and info[:4].cpu().tolist()[2:] == [0, call + 1]


def test_select_triplets_rejects_a_pool_of_one_identity(lib):
    """Every pair of such a pool lacks a negative; the kernel would leave the triplet slots unwritten, so the host refuses."""
    from facenet_amd.triplet import select_triplets
    dist = torch.zeros(8, 8, device="cuda")
    with pytest.raises(ValueError, match="at least two identities"):
        select_triplets(dist, np.zeros(8, dtype=np.int64), 0.2, 4)
    with pytest.raises(ValueError, match="one entry per row"):
        select_triplets(dist, np.zeros(7, dtype=np.int64), 0.2, 4)
