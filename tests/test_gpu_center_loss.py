"""Center loss and prelogits-norm loss of softmax training on the GPU (facenet/facenet.py:204-217,
apps/configs/train_softmax.yaml:73-78; semantics in DESIGN.md section 11, restated in tests/center_loss_oracle.py):
the two kernels through the C ABI, the gradient inside a training step of both model families, the center update over
several eager and captured steps, checkpoints, data parallelism and the app."""
import os
import socket

import numpy as np
import pytest
import torch

from facenet_amd import _lib
from facenet_amd.engine import Network
from facenet_amd.train import Trainer
from tests import center_loss_oracle as co
from tests.util import ptr, stream, structured_images

pytestmark = pytest.mark.gpu

NCLS = 19


@pytest.fixture(autouse=True)
def _heuristic_tiles(monkeypatch):
    # trainers that are compared bit for bit run on the library's deterministic tile heuristic, not on timed choices
    monkeypatch.setenv("FACENET_AUTOTUNE", "0")


def _within_one_ulp(got, want64):
    """got (fp32) is within one fp32 ulp of the float64 value want64."""
    got = np.asarray(got, np.float32)
    return np.all(np.abs(got.astype(np.float64) - want64) <= np.spacing(np.abs(got)).astype(np.float64))


def _labels(N, seed):
    y = np.random.default_rng(seed).integers(0, NCLS, N)
    y[[0, 2, 3]] = 3                                                  # one class three times
    return y


# ---- 1. the kernels through ctypes ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,E,p", [(7, 128, 1.0), (7, 512, 1.5), (100, 128, 2.0), (100, 512, 1.0), (100, 512, 1.5)])
def test_kernels_match_the_oracle(N, E, p):
    lib = _lib.load()
    rng = np.random.default_rng(N * 1000 + E)
    C_, cf, nf, alfa = 37, 0.3, 0.2, 0.95
    x = rng.standard_normal((N, E)).astype(np.float32)
    x[1, :5] = 0.0
    y = np.zeros(N, np.int64)
    y[:] = rng.integers(0, C_, N)
    y[[0, 2, 3, 5, 6]] = 11                                         # class 11 five times
    centers = rng.standard_normal((C_, E)).astype(np.float32)
    demb0 = (rng.standard_normal((N, E)) * 1e-3).astype(np.float32)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    xd, yd, cd, dd = dev(x), dev(y.astype(np.int32)), dev(centers), dev(demb0)
    terms = torch.zeros(8, dtype=torch.float32, device="cuda")
    xy = torch.full((N, E + 1), -7.0, dtype=torch.float32, device="cuda")
    _lib.check(lib.fn_center_loss_fwd_bwd(ptr(xd), ptr(yd), ptr(cd), ptr(dd), ptr(terms), ptr(xy), E + 1, N, E, C_, cf, nf, p,
                                          stream()), "center_loss")
    torch.cuda.synchronize()
    cl, _ = co.center_loss(x, y, centers)
    pn, _ = co.prelogits_norm(x, p)
    t = terms.cpu().numpy()
    assert abs(t[0] - cl) <= 1e-5 * abs(cl) and abs(t[1] - pn) <= 1e-5 * abs(pn), (t[:2], cl, pn)
    assert np.all(t[2:] == 0)                                         # flag and accumulators left zeroed for the next call
    want = demb0.astype(np.float64) + co.regularizer_grad(x, y, centers, cf, nf, p)
    assert _within_one_ulp(dd.cpu().numpy(), want)
    rows = xy.cpu().numpy()
    assert np.array_equal(rows[:, :E], x) and np.array_equal(rows[:, E], y.astype(np.float32))
    _lib.check(lib.fn_center_update(ptr(xy), E + 1, N, E, ptr(cd), C_, alfa, stream()), "center_update")
    torch.cuda.synchronize()
    assert np.array_equal(cd.cpu().numpy(), co.center_update(centers, x, y, alfa))      # bit for bit
    # a factor of 0 adds nothing of its term; the norm is still reported; no centers: no center term
    dd.copy_(dev(demb0))
    _lib.check(lib.fn_center_loss_fwd_bwd(ptr(xd), ptr(yd), None, ptr(dd), ptr(terms), None, 0, N, E, C_, 0.0, 0.0, p, stream()), "")
    torch.cuda.synchronize()
    assert np.array_equal(dd.cpu().numpy(), demb0)
    assert abs(float(terms[1]) - pn) <= 1e-5 * pn
    # a NaN in x: NaN terms, not a silently wrong finite number
    x[4, 9] = np.nan
    xd.copy_(dev(x))
    _lib.check(lib.fn_center_loss_fwd_bwd(ptr(xd), ptr(yd), ptr(cd), ptr(dd), ptr(terms), None, 0, N, E, C_, cf, nf, p, stream()), "")
    torch.cuda.synchronize()
    t = terms.cpu().numpy()
    assert np.isnan(t[0]) and np.isnan(t[1]) and np.all(t[2:] == 0)
    with pytest.raises(ValueError):
        _lib.check(lib.fn_center_update(ptr(xy), E + 1, N, E, ptr(cd), C_, 1.5, stream()), "center_update")


# ---- 2 / 9. the gradient inside a training step, both model families -----------------------------------------------------
def _net(family, seed=0):
    if family == "v1":
        return Network(embedding_size=128, device="cuda:0", nrof_classes=NCLS, train_dtype=torch.float16, seed=seed)
    from facenet_amd.engine_v2 import NetworkV2
    return NetworkV2(128, config={"repeat": [2, 2, 2]}, device="cuda:0", nrof_classes=NCLS, seed=seed)


def _fwd_bwd(tr):
    st = tr.net.stream()
    tr._zero()
    for ops in (tr.plan.fwd, tr.loss_ops, tr.plan.bwd):
        tr.plan.run_ops(ops, st)
    torch.cuda.synchronize()


@pytest.mark.parametrize("family", ["v1", "v2"])
def test_step_gradient_is_xent_plus_regularizers(family):
    N, cf, nf, p = 6, 0.5, 0.05, 1.0
    x = torch.from_numpy(structured_images(N, seed=11))
    y = _labels(N, 5)
    net0, net1 = _net(family), _net(family)          # the same seed: the same parameters (and, for v2, dropout stream)
    assert torch.equal(net0.P, net1.P)
    tr0 = Trainer(net0, batch=N, loss="softmax", lr=0.01)
    tr1 = Trainer(net1, batch=N, loss="softmax", lr=0.01, center_factor=cf, prelogits_norm_factor=nf, prelogits_norm_p=p)
    centers = np.random.default_rng(1).standard_normal(tuple(tr1.centers.shape)).astype(np.float32)
    tr1.centers.copy_(torch.from_numpy(centers))
    for tr in (tr0, tr1):
        tr.set_images(x, torch.from_numpy(y))
        _fwd_bwd(tr)
    emb = tr1.emb.cpu().numpy()
    assert np.array_equal(emb, tr0.emb.cpu().numpy())                 # identical forward passes
    assert tr0.loss_value() == tr1.loss_value()
    want = tr0.demb.cpu().numpy().astype(np.float64) + co.regularizer_grad(emb, y, centers, cf, nf, p)
    assert _within_one_ulp(tr1.demb.cpu().numpy(), want)
    assert float(np.abs(tr1.demb.cpu().numpy() - tr0.demb.cpu().numpy()).max()) > 0
    terms = tr1.loss_terms()
    cl, pn = co.center_loss(emb, y, centers)[0], co.prelogits_norm(emb, p)[0]
    assert abs(terms["center_loss"] - cl) <= 1e-5 * cl and abs(terms["prelogits_norm"] - pn) <= 1e-5 * pn
    assert terms["xent"] == tr1.loss_value()
    assert abs(terms["loss"] - (terms["xent"] + cf * terms["center_loss"] + nf * terms["prelogits_norm"])) <= 1e-9
    assert tr0.loss_terms() == {"xent": tr0.loss_value(), "center_loss": None, "prelogits_norm": None, "loss": tr0.loss_value()}


# ---- 3. several steps: eager, captured, repeated ---------------------------------------------------------------------------
def _run_steps(params, x, y, graph, steps=3, alfa=0.9):
    net = _net("v1", seed=3)
    net.load_keras_params(params)
    tr = Trainer(net, batch=len(y), loss="softmax", lr=0.01, center_factor=0.1, center_alfa=alfa, prelogits_norm_factor=0.01)
    tr.set_images(x, torch.from_numpy(y))
    if graph:
        tr.centers.fill_(0.25)
        tr.capture()
        torch.cuda.synchronize()
        assert torch.all(tr.centers == 0.25)                          # capture() leaves the centers untouched
        tr.centers.zero_()
    embs, cents = [], []
    for _ in range(steps):
        tr.step()
        torch.cuda.synchronize()
        embs.append(tr.emb.cpu().numpy().copy())
        cents.append(tr.centers.cpu().numpy().copy())
    return embs, cents, net.P.cpu().numpy()


def test_centers_follow_the_update_over_steps_eager_and_captured():
    N, alfa = 6, 0.9
    x = torch.from_numpy(structured_images(N, seed=12))
    y = _labels(N, 8)
    params = _net("v1").export_keras_params()
    eager = _run_steps(params, x, y, graph=False, alfa=alfa)
    c = np.zeros((NCLS, 128), np.float32)
    for emb, got in zip(*eager[:2]):
        c = co.center_update(c, emb, y, alfa)
        assert np.array_equal(got, c)
    assert float(np.abs(c).max()) > 0
    captured = _run_steps(params, x, y, graph=True, alfa=alfa)
    again = _run_steps(params, x, y, graph=True, alfa=alfa)
    for run in (captured, again):
        for a, b in zip(eager[0] + eager[1] + [eager[2]], run[0] + run[1] + [run[2]]):
            assert np.array_equal(a, b)


# ---- 4. factors at 0 -------------------------------------------------------------------------------------------------------
def test_factors_at_zero_are_todays_trainer():
    x = torch.from_numpy(structured_images(4, seed=13))
    y = torch.tensor([1, 5, 5, 18])
    params = _net("v1").export_keras_params()
    trs = []
    for kw in ({}, dict(center_factor=0.0, center_alfa=0.5, prelogits_norm_factor=0.0, prelogits_norm_p=2.0)):
        net = _net("v1", seed=1)
        net.load_keras_params(params)
        tr = Trainer(net, batch=4, loss="softmax", lr=0.01, **kw)
        tr.set_images(x, y)
        tr.step()
        torch.cuda.synchronize()
        trs.append(tr)
    a, b = trs
    assert [op.name for op in a.step_ops] == [op.name for op in b.step_ops]
    assert b.centers is None and not b.regularized and not hasattr(b, "reg_terms")
    assert torch.equal(a.G, b.G) and torch.equal(a.net.P, b.net.P)
    assert b.loss_terms()["center_loss"] is None and b.loss_terms()["loss"] == b.loss_value()


# ---- 5. errors -------------------------------------------------------------------------------------------------------------
def test_invalid_settings_raise():
    net = _net("v1")
    for kw in (dict(center_factor=0.01), dict(prelogits_norm_factor=0.01)):
        with pytest.raises(ValueError):
            Trainer(net, batch=6, loss="triplet", **kw)
    for kw in (dict(center_factor=0.1, center_alfa=-0.1), dict(center_factor=0.1, center_alfa=1.5), dict(prelogits_norm_p=0.0),
               dict(prelogits_norm_factor=0.1, prelogits_norm_p=-1.0), dict(center_factor=-0.1), dict(prelogits_norm_factor=-1.0)):
        with pytest.raises(ValueError):
            Trainer(net, batch=4, loss="softmax", **kw)


# ---- 6. checkpoints --------------------------------------------------------------------------------------------------------
def test_checkpoint_round_trip_with_centers(tmp_path):
    x = torch.from_numpy(structured_images(4, seed=14))
    y = torch.tensor([2, 2, 9, 2])
    params = _net("v1").export_keras_params()
    kw = dict(batch=4, loss="softmax", lr=0.01, center_factor=0.2, prelogits_norm_factor=0.01)

    def trainer(seed, **extra):
        net = _net("v1", seed=seed)
        net.load_keras_params(params)
        tr = Trainer(net, **dict(kw, **extra))
        tr.set_images(x, y)
        return tr

    tr = trainer(0)
    tr.step()
    path = tmp_path / "ckpt.npz"
    tr.save_checkpoint(path, epoch=1)
    tr.step()
    torch.cuda.synchronize()
    with np.load(path) as z:
        assert z["centers:0"].shape == (NCLS, 128) and float(np.abs(z["centers:0"]).max()) > 0
    tr2 = trainer(5)
    assert tr2.load_checkpoint(path) == 1
    tr2.step()
    torch.cuda.synchronize()
    assert torch.equal(tr.centers, tr2.centers)
    a, b = tr.net.export_keras_params(), tr2.net.export_keras_params()
    for k in a:
        assert torch.equal(a[k], b[k]), k
    # a checkpoint without centers:0 loads with zero centers; a trainer without center loss ignores the key
    with np.load(path) as z:
        sd = {k: z[k] for k in z.files if k != "centers:0"}
    plain = tmp_path / "plain.npz"
    np.savez(plain, **sd)
    tr3 = trainer(6)
    tr3.centers.fill_(1.0)
    tr3.load_checkpoint(plain)
    assert float(tr3.centers.abs().max()) == 0.0
    tr4 = trainer(7, center_factor=0.0)
    assert tr4.centers is None
    assert tr4.load_checkpoint(path) == 1
    assert "centers:0" not in tr4.state_dict()


# ---- 7. data parallelism ---------------------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _rank(rank, world, port, q, use_graph):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["FACENET_AUTOTUNE"] = "0"
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        net = Network(embedding_size=128, device="cuda:0", nrof_classes=NCLS, train_dtype=torch.float16, seed=0)
        tr = Trainer(net, batch=4, loss="softmax", lr=0.01, world_size=world, process_group=dist.group.WORLD, n_buckets=4,
                     center_factor=0.1, center_alfa=0.8, prelogits_norm_factor=0.01)
        y = np.array([[4, 7, 4, 0], [7, 4, 12, 4]][rank])          # class 4 on both ranks, twice on each
        tr.set_images(torch.from_numpy(structured_images(4, seed=50 + rank)), torch.from_numpy(y))
        if use_graph:
            tr.capture()
        embs, cents = [], []
        for _ in range(2):
            tr.step()
            torch.cuda.synchronize()
            embs.append(tr.emb.cpu().numpy().copy())
            cents.append(tr.centers.cpu().numpy().copy())
        q.put((rank, y, embs, cents, net.P.cpu().numpy()))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("use_graph", [False, True])
def test_two_replicas_keep_identical_centers(use_graph):
    import torch.multiprocessing as mp
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_rank, args=(r, world, port, q, use_graph)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=600) for _ in range(world)], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    assert np.array_equal(res[0][4], res[1][4])
    c = np.zeros((NCLS, 128), np.float32)
    y = np.concatenate([res[0][1], res[1][1]])                       # the global batch in rank order
    for s in range(2):
        assert np.array_equal(res[0][3][s], res[1][3][s])            # bitwise equal on both ranks
        c = co.center_update(c, np.concatenate([res[0][2][s], res[1][2][s]]), y, 0.8)
        assert np.array_equal(res[0][3][s], c)
    assert float(np.abs(c).max()) > 0


# ---- 8. the app ------------------------------------------------------------------------------------------------------------
def test_train_softmax_app_logs_the_regularizers():
    from facenet_amd.apps.train_softmax import train_softmax
    from facenet_amd.config import load_config
    logs = []
    cfg = load_config(overrides={"batch_size": 8, "loss": {"center_factor": 0.01, "prelogits_norm_factor": 5e-4},
                                 "train": {"epoch": {"nrof_epochs": 2, "size": 4}, "learning_rate": {"value": 0.01}}})
    x = torch.from_numpy(structured_images(8, seed=4))
    y = torch.from_numpy(np.random.default_rng(5).integers(0, 37, 8))
    net, tr = train_softmax(cfg, 37, batches=((x, y) for _ in iter(int, 1)), embedding_size=128, log=logs.append)
    assert len(logs) == 2 and tr.centers is not None
    vals = [{k: float(line.split(f"  {k} ")[1].split()[0]) for k in ("xent", "center_loss", "prelogits_norm", "loss")} for line in logs]
    for v in vals:
        assert all(np.isfinite(list(v.values())))
        assert v["loss"] > v["xent"]
    assert tr.loss_value() < vals[0]["xent"]
