"""fn_batch_triplet_fwd_bwd, its head in the Trainer and the app on the GPU.  The kernel and the fp64 oracle
(tests/batch_triplet_oracle.py) both consume the distance matrix fn_pairwise_sqdist wrote on the device: every mining decision is
taken on the same bits, so a hinge's coef and info are compared exactly and loss, soft coef and demb under their derived bounds."""
import os
import socket

import numpy as np
import pytest
import torch

from facenet_amd import _lib
from facenet_amd.engine import Network
from facenet_amd.train import Trainer
from oracle import facenet_oracle as fo
from tests import batch_triplet_oracle as bo
from tests import elementwise_oracle as eo
from tests import pair_lattice as pl
from tests.util import ptr, stream
from tests.util_data import structured_images

pytestmark = pytest.mark.gpu

SETTINGS = [(0, 0), (0, 1), (1, 0), (1, 1)]                            # (strategy, soft)
POISON, TAIL = 7.25, 16


def _rows(n, E, seed, scale=1.5):
    """Rows of norm ``scale``: the kernel must not assume unit norm."""
    x = np.random.default_rng(seed).standard_normal((n, E))
    return (scale * x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def _call(lib, x, labels, alpha, strategy, soft, with_grad=True, poke=None):
    """One call over poisoned buffers with a guard tail -> dict of host arrays (dist: what the device wrote and the kernel read;
    ``poke(dist)`` may edit it on the device in between)."""
    n, E = x.shape
    emb = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    dist = torch.empty(n, n, device="cuda")
    _lib.check(lib.fn_pairwise_sqdist(ptr(emb), ptr(emb), ptr(dist), None, n, n, E, 2, stream()))
    if poke is not None:
        poke(dist)
    lab = torch.from_numpy(np.asarray(labels).astype(np.int32)).cuda()
    coef = torch.full((n * n + TAIL,), POISON, device="cuda")
    demb = torch.full((n * E + TAIL,), POISON, device="cuda")
    loss = torch.full((4,), POISON, device="cuda")
    info = torch.full((8 + TAIL,), 77, dtype=torch.int32, device="cuda")
    _lib.check(lib.fn_batch_triplet_fwd_bwd(ptr(emb), ptr(dist), ptr(lab), ptr(demb) if with_grad else None, ptr(loss), ptr(coef), ptr(info),
                                            n, E, alpha, strategy, soft, stream()))
    torch.cuda.synchronize()
    assert bool((coef[n * n:] == POISON).all()) and bool((info[8:] == 77).all()) and bool((demb[n * E:] == POISON).all())
    if not with_grad:
        assert bool((demb == POISON).all())
    return dict(dist=dist.cpu().numpy(), coef=coef[:n * n].view(n, n).cpu().numpy(), demb=demb[:n * E].view(n, E).cpu().numpy(),
                loss=loss.cpu().numpy(), info=info[:8].cpu().numpy())


def _check(got, o, soft, what, with_grad=True):
    assert np.array_equal(got["info"], o["info"]), (what, got["info"], o["info"])
    if soft:
        eo.check_bound(got["coef"], o["coef"], o["e_coef"], what + " coef")
        assert np.array_equal(got["coef"] == 0, o["coef"] == 0)
    else:
        assert np.array_equal(got["coef"], o["coef"]), what + " coef"
    print(f"{what}: loss {got['loss'][0]:.9g} fp64 {o['loss']:.12g} bound {o['e_loss']:.3g}")
    eo.check_bound(got["loss"][0], o["loss"], o["e_loss"], what + " loss")
    if with_grad:
        eo.check_bound(got["demb"], o["demb"], o["e_demb"], what + " demb")


# ---- 1. degenerate batches and the smallest live one ---------------------------------------------------------------------------
@pytest.mark.parametrize("strategy,soft", SETTINGS)
@pytest.mark.parametrize("labels", [[0, 0], [0, 1]])
def test_degenerate_batches_write_zeros(lib, labels, strategy, soft):
    got = _call(lib, _rows(2, 5, 1), labels, 0.2, strategy, soft)
    assert not got["info"].any() and got["loss"][0] == 0.0
    assert not got["coef"].any() and not got["demb"].any()


@pytest.mark.parametrize("strategy,soft", SETTINGS)
def test_smallest_live_batch(lib, strategy, soft):
    """N = 3, labels (0, 0, 1): row 2 is nobody's anchor (a zero row of coef) and still gets a gradient, as a negative.  alpha = 10
    is above every distance of rows of norm 1.5 (<= 9), so both hinges are active."""
    x = _rows(3, 3, 2)
    got = _call(lib, x, [0, 0, 1], 10.0, strategy, soft)
    o = bo.mine(got["dist"], [0, 0, 1], 10.0, strategy, soft, emb=x)
    _check(got, o, soft, "N=3")
    assert list(got["info"][:3]) == [2, 2, 2] and not got["coef"][2].any()
    assert np.abs(got["demb"][2]).max() > 0 and got["coef"][0, 1] > 0 > got["coef"][0, 2]


# ---- 2. shapes -------------------------------------------------------------------------------------------------------------------
# N: one partial wave, a ragged chunk, one and two waves, a second chunk of 256; E: below a lane row, the 64 / 65 lane boundary, the
# production 128, the 512 limit (two trips of the gather's 256-wide e loop)
SHAPES = [(4, 3), (7, 65), (64, 64), (65, 128), (257, 512), (257, 3)]


@pytest.mark.parametrize("strategy,soft", SETTINGS)
@pytest.mark.parametrize("n,E", SHAPES)
def test_shapes_ragged_classes(lib, n, E, strategy, soft):
    labels = bo.ragged_labels(n, seed=n + E)                          # sizes 1, 2, 3, 7, ...: unsorted, non-contiguous, negative ids
    x = _rows(n, E, seed=n * 1000 + E)
    got = _call(lib, x, labels, 0.2, strategy, soft)
    assert np.array_equal(got["dist"], got["dist"].T)
    o = bo.mine(got["dist"], labels, 0.2, strategy, soft, emb=x)
    assert o["Z"] > 0 and (soft or 0 < o["info"][2])
    _check(got, o, soft, f"N={n} E={E} strategy={strategy} soft={soft}")
    loss_only = _call(lib, x, labels, 0.2, strategy, soft, with_grad=False)          # demb = NULL
    for k in ("loss", "coef", "info"):
        assert np.array_equal(loss_only[k].view(np.uint32), got[k].view(np.uint32)), k


def test_wrapper_returns_loss_gradient_and_info(lib):
    from facenet_amd.triplet import batch_triplet_loss
    n, E = 30, 128
    labels, x = bo.ragged_labels(n, 3), _rows(n, E, 9, scale=1.0)
    got = _call(lib, x, labels, 0.3, 1, 0)
    loss, grad, info = batch_triplet_loss(torch.from_numpy(x).cuda(), labels, alpha=0.3, strategy="batch_all", with_grad=True)
    assert float(loss) == got["loss"][0] and np.array_equal(grad.cpu().numpy(), got["demb"])
    assert [info["anchors"], info["terms"], info["active"]] == list(got["info"][:3]) and info["active_fraction"] == info["active"] / info["terms"]
    loss2, info2 = batch_triplet_loss(torch.from_numpy(x).cuda(), labels, strategy="batch_hard", soft=True)
    assert np.isfinite(float(loss2)) and info2["active"] == info2["terms"] == info2["anchors"]
    with pytest.raises(ValueError, match="unknown strategy"):
        batch_triplet_loss(torch.from_numpy(x).cuda(), labels, strategy="semi_hard")


# ---- 3. ties and exact zeros ---------------------------------------------------------------------------------------------------
def test_lattice_ties_and_exact_zero_hinges(lib):
    """Lattice rows: every distance is h / 16 exactly (h the Hamming distance), so with alpha = 1 the hinge of a triplet with
    h_an - h_ap = 16 is exactly 0: inactive, in neither info[2] nor coef.  Row 1 duplicates row 0, so for anchors of other classes
    the two tie bitwise and the lowest index must win."""
    sizes = [5, 4, 6, 3]
    x, _, H = pl.lattice_classes(sizes, seed=3, flips=8)
    labels = np.repeat(np.arange(len(sizes)), sizes)
    n = len(labels)
    same = (labels[:, None] == labels[None, :]) & ~np.eye(n, dtype=bool)
    l16 = H[:, :, None] - H[:, None, :] + 16                            # [a, p, n]: 16 (d_ap - d_an + 1)
    valid = same[:, :, None] & (labels[:, None] != labels[None, :])[:, None, :]
    assert int((valid & (l16 == 0)).sum()) == 10                        # the planted exact zeros
    got = _call(lib, x, labels, 1.0, 1, 0)
    assert np.array_equal(got["dist"], (H / 16.0).astype(np.float32))
    assert list(got["info"][:4]) == [n, int(valid.sum()), int((valid & (l16 > 0)).sum()), 0]
    act = valid & (l16 > 0)
    want = act.sum(2) - act.sum(1)                                      # [a, p]: its active negatives; [a, n]: minus its active positives
    assert np.array_equal(got["coef"], want.astype(np.float32))
    _check(got, bo.mine(got["dist"], labels, 1.0, 1, 0, emb=x), 0, "lattice batch all")
    for soft in (0, 1):
        hard = _call(lib, x, labels, 1.0, 0, soft)
        _check(hard, bo.mine(hard["dist"], labels, 1.0, 0, soft, emb=x), soft, "lattice batch hard")
        tied = [a for a in range(sizes[0], n) if H[a, 0] == H[a, labels != labels[a]].min()]
        if soft:
            assert tied and all(hard["coef"][a, 0] < 0 and hard["coef"][a, 1] == 0 for a in tied)
    # row 2 is row 0 negated and row 3 differs in 32 places: anchor 1's farthest positive is 2, and rows 0, 1 tie as anchor 2's
    soft_hard = _call(lib, x, labels, 1.0, 0, 1)
    assert soft_hard["coef"][1, 2] > 0 and soft_hard["coef"][2, 0] > 0 and soft_hard["coef"][2, 1] == 0


# ---- 4. range --------------------------------------------------------------------------------------------------------------------
def test_batch_all_at_the_row_limit_keeps_the_loss_sum(lib):
    """N = 1024, K = 4, E = 128, batch all with a hinge: 3.1 M terms whose un-normalised sum is past 2^23, where a 40-fractional-bit
    fixed-point accumulator wraps."""
    n, E = 1024, 128
    labels = np.random.default_rng(1).permutation(np.repeat(np.arange(n // 4), 4))
    x = _rows(n, E, 7, scale=6.0)
    got = _call(lib, x, labels, 0.2, 1, 0)
    o = bo.mine(got["dist"], labels, 0.2, 1, 0, emb=x)
    assert o["info"][1] == n * 3 * (n - 4) and o["loss"] * o["Z"] > 2.0 ** 23
    _check(got, o, 0, "N=1024")


def test_limits_and_bad_settings_are_refused(lib):
    n, E = 4, 8
    bufs = [torch.zeros(1100 * 1100, device="cuda") for _ in range(5)]
    emb, dist, demb, loss, coef = bufs
    lab, info = torch.zeros(1100, dtype=torch.int32, device="cuda"), torch.zeros(8, dtype=torch.int32, device="cuda")

    def call(n=n, E=E, alpha=0.2, strategy=0, soft=0, null=None):
        a = dict(emb=ptr(emb), dist=ptr(dist), labels=ptr(lab), demb=ptr(demb), loss=ptr(loss), coef=ptr(coef), info=ptr(info))
        if null:
            a[null] = None
        _lib.check(lib.fn_batch_triplet_fwd_bwd(a["emb"], a["dist"], a["labels"], a["demb"], a["loss"], a["coef"], a["info"], n, E, alpha,
                                                strategy, soft, stream()))
    call()
    call(alpha=-1.0, soft=1)                                           # alpha is ignored under a soft margin
    call(null="demb")
    for kw in (dict(n=1025), dict(n=1), dict(E=513), dict(E=0), dict(alpha=-0.1), dict(alpha=float("nan")), dict(alpha=float("inf")),
               dict(strategy=2), dict(strategy=-1), dict(soft=2), dict(null="emb"), dict(null="dist"), dict(null="labels"),
               dict(null="loss"), dict(null="coef"), dict(null="info")):
        with pytest.raises(ValueError):
            call(**kw)
    torch.cuda.synchronize()


# ---- 5. non-finite input, reproducibility ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("strategy,soft", SETTINGS)
def test_a_nan_row_makes_the_loss_nan(lib, strategy, soft):
    """A NaN row (and, the matrix being symmetric, column) of dist.  It is planted in dist itself: fn_pairwise_sqdist's final
    max(., 0) turns a NaN embedding into a distance of 0, so a NaN can reach the kernel only through a matrix made elsewhere."""
    def poke(dist):
        dist[3, :] = float("nan")
        dist[:, 3] = float("nan")
    got = _call(lib, _rows(9, 16, 4), [0, 0, 0, 1, 1, 1, 2, 2, 2], 0.2, strategy, soft, poke=poke)
    assert got["info"][3] == 1 and np.isnan(got["loss"][0]) and not got["info"][4:].any()
    clean = _call(lib, _rows(9, 16, 4), [0, 0, 0, 1, 1, 1, 2, 2, 2], 0.2, strategy, soft)
    assert clean["info"][3] == 0 and np.isfinite(clean["loss"][0])


@pytest.mark.parametrize("strategy,soft", SETTINGS)
def test_same_call_same_bits(lib, strategy, soft):
    n, E = 180, 128
    labels, x = np.repeat(np.arange(45), 4), _rows(n, E, 5, scale=1.0)
    a, b = (_call(lib, x, labels, 0.2, strategy, soft) for _ in range(2))
    for k in ("loss", "coef", "demb", "info"):
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k


# ---- 6. the Trainer --------------------------------------------------------------------------------------------------------------
HEAD_OPS = ["l2norm_fwd", "pairwise_sqdist", "batch_triplet", "l2norm_bwd"]
P_, K_ = 4, 3
LABELS = np.repeat(np.array([11, -4, 7, 300]), K_)


def _net(family, seed=0):
    if family == "v1":
        return Network(embedding_size=128, device="cuda:0", train_dtype=torch.float16, seed=seed)
    from facenet_amd.engine_v2 import NetworkV2
    return NetworkV2(128, config={"repeat": [2, 2, 2]}, device="cuda:0", seed=seed)


@pytest.mark.parametrize("family,strategy,soft", [("v1", "batch_all", False), ("v2", "batch_hard", True)])
def test_step_stage_by_stage(family, strategy, soft):
    N = P_ * K_
    net = _net(family)
    tr = Trainer(net, batch=N, loss="triplet", alpha=0.2, lr=0.01, triplet_strategy=strategy, soft_margin=soft)
    assert [op.name for op in tr.loss_ops] == HEAD_OPS and tr.head.state == ()
    labels = np.random.default_rng(2).permutation(LABELS)
    tr.set_images(torch.from_numpy(structured_images(N, seed=21)), labels)
    st = net.stream()
    tr._zero()
    for ops in (tr.plan.fwd, tr.loss_ops, tr.plan.bwd):
        tr.plan.run_ops(ops, st)
    torch.cuda.synchronize()
    emb, embn, dist = tr.emb.cpu(), tr.embn.cpu(), tr.dist.cpu().numpy()
    ref, bound, _, _ = eo.l2norm_ref(emb, 1e-10)
    eo.check_bound(embn, ref, bound, "embn")
    assert np.array_equal(dist, fo.squared_distance_matrix(embn.numpy())) and np.array_equal(dist, dist.T)
    code = (0 if strategy == "batch_hard" else 1, 1 if soft else 0)
    o = bo.mine(dist, labels, 0.2, *code, emb=embn.numpy())
    got = dict(info=tr.mine_info.cpu().numpy(), coef=tr.coef.cpu().numpy(), loss=tr.loss.cpu().numpy(), demb=tr.dembn.cpu().numpy())
    assert o["info"][0] == N and o["Z"] > 0
    _check(got, o, code[1], f"{family} {strategy}")
    assert tr.loss_value() == float(got["loss"][0])
    stats = tr.triplet_stats()
    assert [stats["anchors"], stats["terms"], stats["active"]] == list(o["info"][:3]) and stats["active_fraction"] == o["info"][2] / o["info"][1]
    ref, bound, ok = eo.l2norm_bwd_ref(emb, tr.dembn.cpu(), 1e-10)
    assert ok
    eo.check_bound(tr.demb.cpu(), ref, bound, "demb")
    assert float(tr.demb.abs().amax(dim=1).min()) > 0                   # every embedded image receives a gradient
    assert float(tr.G.abs().max()) > 0 and bool(torch.isfinite(tr.G).all())


def test_set_images_checks_labels_and_other_heads_refuse():
    net = _net("v1")
    tr = Trainer(net, batch=6, loss="triplet", lr=0.01, triplet_strategy="batch_hard")
    x = torch.from_numpy(structured_images(6, seed=1))
    with pytest.raises(ValueError, match="one identity per batch row"):
        tr.set_images(x, [0, 0, 1])
    for bad in ([3] * 6, [0, 1, 2, 3, 4, 5]):                          # no negative; no positive
        with pytest.raises(ValueError, match="both a positive and a negative"):
            tr.set_images(x, bad)
    tr.set_images(x, torch.tensor([5, 5, -2, 9, 9, 9]))
    assert tr.labels.dtype == torch.int32 and tr.labels.cpu().tolist() == [5, 5, -2, 9, 9, 9]
    mined = Trainer(net, batch=6, loss="triplet", lr=0.01)
    with pytest.raises(ValueError, match="labels are only used by the softmax loss"):
        mined.set_images(x, [0, 0, 1, 1, 2, 2])
    with pytest.raises(RuntimeError, match="triplet_stats"):
        mined.triplet_stats()


def _label_sets(steps, seed):
    rng = np.random.default_rng(seed)
    return [rng.permutation(LABELS) for _ in range(steps)]


def _run_steps(params, x, graph, steps=3, strategy="batch_all", soft=False, **kw):
    net = _net("v1", seed=3)
    net.load_keras_params(params)
    tr = Trainer(net, batch=len(x), loss="triplet", lr=0.01, triplet_strategy=strategy, soft_margin=soft, **kw)
    labels = _label_sets(steps, 6)
    tr.set_images(x, labels[0])
    if graph:
        tr.capture()
    out = []
    for s in range(steps):
        tr.set_images(x, labels[s])                                     # labels live on the device: a replay sees the new ones
        tr.step()
        torch.cuda.synchronize()
        out += [tr.emb.cpu().numpy().copy(), tr.coef.cpu().numpy().copy(), tr.loss.cpu().numpy()[:1].copy()]
    assert np.isfinite(tr.loss_value())
    return out + [net.P.cpu().numpy()], tr


def test_three_steps_eager_and_captured_are_bitwise_equal():
    x = torch.from_numpy(structured_images(P_ * K_, seed=22))
    params = _net("v1").export_keras_params()
    eager, _ = _run_steps(params, x, graph=False)
    assert float(np.abs(eager[0] - eager[6]).max()) > 0                # the steps move the embedding
    assert not np.array_equal(eager[1], eager[4])                      # and the changed labels change the mining
    captured, _ = _run_steps(params, x, graph=True)
    for a, b in zip(eager, captured):
        assert np.array_equal(a, b)


def test_mined_trainer_is_untouched_by_a_batch_trainer_in_the_process():
    x = torch.from_numpy(structured_images(6, seed=23))
    params = _net("v1").export_keras_params()

    def mined(**kw):
        net = _net("v1", seed=1)
        net.load_keras_params(params)
        tr = Trainer(net, batch=6, loss="triplet", alpha=0.2, lr=0.01, **kw)
        tr.set_images(x)
        for _ in range(2):
            tr.step()
        torch.cuda.synchronize()
        return tr

    a = mined()
    _run_steps(params, torch.from_numpy(structured_images(P_ * K_, seed=22)), graph=False, steps=1, strategy="batch_hard", soft=True)
    b = mined(triplet_strategy="mined")
    assert [op.name for op in a.step_ops] == [op.name for op in b.step_ops] and "triplet_loss" in [op.name for op in b.step_ops]
    assert not hasattr(b, "coef") and float(a.G.abs().max()) > 0
    assert torch.equal(a.G, b.G) and torch.equal(a.net.P, b.net.P) and torch.equal(a.loss[:1], b.loss[:1])


def test_checkpoint_round_trip(tmp_path):
    x = torch.from_numpy(structured_images(P_ * K_, seed=24))
    params = _net("v1").export_keras_params()

    def trainer(seed):
        net = _net("v1", seed=seed)
        net.load_keras_params(params)
        tr = Trainer(net, batch=P_ * K_, loss="triplet", lr=0.01, triplet_strategy="batch_hard")
        tr.set_images(x, LABELS)
        return tr

    tr = trainer(0)
    keys = set(tr.state_dict())
    tr.step()
    path = tmp_path / "ckpt.npz"
    tr.save_checkpoint(path, epoch=1)
    tr.step()
    torch.cuda.synchronize()
    with np.load(path) as z:
        assert set(z.files) == keys                                     # the head adds no state
    tr2 = trainer(5)
    assert tr2.load_checkpoint(path) == 1
    tr2.step()
    torch.cuda.synchronize()
    a, b = tr.net.export_keras_params(), tr2.net.export_keras_params()
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert torch.equal(tr.loss[:1], tr2.loss[:1])


# ---- 7. the one-rank process group ---------------------------------------------------------------------------------------------
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
        x = torch.from_numpy(structured_images(P_ * K_, seed=25))
        out, tr = _run_steps(params, x, graph=False, steps=2, strategy="batch_hard", world_size=1, process_group=dist.group.WORLD, n_buckets=4)
        assert tr.exchange and len(tr.segments) == len(tr.buckets) + 1
        q.put((out[-1], tr.G.cpu().numpy(), tr.loss_value()))
    finally:
        dist.destroy_process_group()


def test_one_rank_process_group_equals_the_plain_step():
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_one_rank, args=(_free_port(), q))
    p.start()
    try:
        P, G, loss = q.get(timeout=600)
        p.join(timeout=120)
        assert p.exitcode == 0
    finally:
        if p.is_alive():
            p.kill()
    params, _, _ = fo.build_params(128, seed=0)
    x = torch.from_numpy(structured_images(P_ * K_, seed=25))
    out, tr = _run_steps(params, x, graph=False, steps=2, strategy="batch_hard")
    assert float(np.abs(G).max()) > 0
    assert np.array_equal(G, tr.G.cpu().numpy()) and np.array_equal(P, out[-1]) and loss == tr.loss_value()


# ---- 8. the app --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strategy", ["batch_hard", "batch_all"])
def test_app_runs_an_epoch_and_logs_the_active_fraction(strategy):
    from facenet_amd.apps.train_tripletloss import train_tripletloss
    from facenet_amd.config import load_config
    logs = []
    cfg = load_config(overrides={"loss": {"triplet_strategy": strategy}, "train": {"epoch": {"nrof_epochs": 1, "size": 2},
                                                                                   "learning_rate": {"value": 0.01}}})
    x = torch.from_numpy(structured_images(P_ * K_, seed=26))
    pools = iter([x, (x, LABELS[::-1].copy())])
    net, tr = train_tripletloss(cfg, people_per_batch=P_, images_per_person=K_, pools=pools, log=logs.append)
    assert logs[0] == f"triplet strategy: {strategy}" and len(logs) == 2
    assert tr.N == P_ * K_ and tr.triplet_strategy == strategy and tr._graph is not None
    names = [op.name for op in tr.step_ops]
    assert "batch_triplet" in names and "triplet_loss" not in names
    line = logs[1]
    assert np.isfinite(float(line.split("triplet loss ")[1].split()[0]))
    frac = float(line.split("active ")[1].split()[0])
    stats = tr.triplet_stats()
    assert 0 < frac <= 1 and abs(frac - stats["active_fraction"]) <= 5e-4 and f"({stats['active']}/{stats['terms']})" in line
    assert tr.labels.cpu().tolist() == LABELS[::-1].tolist()
