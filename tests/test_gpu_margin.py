"""The large-margin cosine softmax (NormFace / CosFace / ArcFace) on the GPU: the three kernels through the
C ABI against the fp64 oracle and its derived bounds (tests/margin_oracle.py), one training step of both model families checked
stage by stage on the operands the device itself produced, the regularisers on top, reproducibility eager / captured, the plain
trainer left as it is, data parallelism, checkpoints and the app."""
import os
import socket

import numpy as np
import pytest
import torch

from facenet_amd import _lib
from facenet_amd.engine import Network
from facenet_amd.train import Trainer
from tests import center_loss_oracle as co
from tests import elementwise_oracle as eo
from tests import margin_oracle as mo
from tests.util import ACC_GRAD_BITS, assert_elementwise, bitpattern, ptr, same_bits, stream, structured_images, wgrad_k

pytestmark = pytest.mark.gpu
BF, HF = _lib.FN_BF16, _lib.FN_F16
JUNK = 0x5A5A5A5A5A5A
NCLS = 19
MARGIN_OPS = ["l2norm_fwd", "cast_emb", "margin_rnorm", "conv_fwd:classifier", "margin_softmax", "conv_wgrad:classifier",
              "margin_wgrad_fix", "conv_dgrad:classifier", "l2norm_bwd"]


@pytest.fixture(autouse=True)
def _heuristic_tiles(monkeypatch):
    # trainers that are compared bit for bit run on the library's deterministic tile heuristic, not on timed choices
    monkeypatch.setenv("FACENET_AUTOTUNE", "0")


_INPUTS = {}


def _case(N, C, ld, setting, dt):
    """Inputs and fp64 reference of one (shape, setting, dtype): computed once, shared, never modified."""
    key = (N, C, ld, setting, dt)
    if key not in _INPUTS:
        z, r, labels = mo.margin_inputs(N, C, ld, seed=N, m_arc=setting[1])
        ref = mo.margin_ref(z, r, labels, C, *setting, 1.0 / N, dt)
        assert ref["margin_ok"]
        _INPUTS[key] = (z, r, labels, ref)
    return _INPUTS[key]


# ---- 1. fn_margin_softmax_fwd_bwd ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [BF, HF])
@pytest.mark.parametrize("setting", mo.SETTINGS)
@pytest.mark.parametrize("N,C,ld,ld_d", mo.SHAPES)
def test_margin_softmax_edges(lib, N, C, ld, ld_d, setting, dt):
    """Every branch of the label column on purpose (margin_inputs), padding columns of z and rnorm poisoned, dz's padding columns
    zero up to ld_d and untouched beyond, t untouched beyond C, dz = NULL, t = NULL."""
    z, r, labels, ref = _case(N, C, ld, setting, dt)
    zd, rd, ld_dev = z.cuda(), r.cuda(), labels.cuda()
    for with_dz, with_t in ((True, True), (True, False), (False, True), (False, False)):
        loss = torch.full((4,), 7.0, device="cuda")
        dz = bitpattern((N * ld_d + 16,), dt)
        before = dz.clone()
        t = torch.zeros(C + 8, dtype=torch.int64, device="cuda")
        t[C:] = JUNK
        _lib.check(lib.fn_margin_softmax_fwd_bwd(ptr(zd), ld, ptr(rd), ptr(ld_dev), ptr(loss), ptr(dz) if with_dz else None, ld_d,
                                                 ptr(t) if with_t else None, N, C, *setting, 1.0 / N, dt, stream()))
        torch.cuda.synchronize()
        eo.check_bound(loss[0], ref["loss"], ref["e_loss"], "margin loss")
        if with_dz:
            got = dz[:N * ld_d].view(N, ld_d).cpu()
            eo.check_bound(got[:, :C], ref["dz"], ref["e_dz"], "dz")
            assert float(got[:, C:].float().abs().max()) == 0, "padding columns of dz"
            assert same_bits(dz[N * ld_d:], before[N * ld_d:])
        else:
            assert same_bits(dz, before)
        if with_t:
            eo.check_bound(t[:C].cpu().double() * 2.0 ** -ACC_GRAD_BITS, ref["t"], ref["e_t"], "t")
        else:
            assert int(t[:C].abs().max()) == 0
        assert bool((t[C:] == JUNK).all())


def test_margin_softmax_invalid_label_and_settings(lib):
    N, C, ld, ld_d = mo.SHAPES[0]
    setting = mo.SETTINGS[0]
    z, r, labels, ref = _case(N, C, ld, setting, HF)
    zd, rd = z.cuda(), r.cuda()
    loss = torch.zeros(4, device="cuda")
    dz = torch.zeros(N, ld_d, dtype=torch.float16, device="cuda")
    t = torch.zeros(C, dtype=torch.int64, device="cuda")
    for bad in (C, -1):
        lab = labels.clone()
        lab[5] = bad                                                          # row 5 is no deliberate case
        ld_dev = lab.cuda()
        _lib.check(lib.fn_margin_softmax_fwd_bwd(ptr(zd), ld, ptr(rd), ptr(ld_dev), ptr(loss), ptr(dz), ld_d, ptr(t), N, C, *setting,
                                                 1.0 / N, HF, stream()))
        torch.cuda.synchronize()
        assert bool(torch.isnan(loss[0]))
        assert bool((dz[5, :C].float() >= 0).all()) and bool(torch.isfinite(dz.float()).all())      # no one-hot term in that row
    ld_dev = labels.cuda()
    for s, m2, m3 in ((0.0, 0.5, 0.0), (-1.0, 0.0, 0.0), (64.0, -0.1, 0.0), (64.0, float(np.pi / 2), 0.0), (64.0, 2.0, 0.0),
                      (64.0, 0.5, -0.1), (float("nan"), 0.0, 0.0)):
        with pytest.raises(ValueError):
            _lib.check(lib.fn_margin_softmax_fwd_bwd(ptr(zd), ld, ptr(rd), ptr(ld_dev), ptr(loss), ptr(dz), ld_d, ptr(t), N, C, s, m2, m3,
                                                     1.0 / N, HF, stream()))
    with pytest.raises(ValueError):
        _lib.check(lib.fn_margin_softmax_fwd_bwd(ptr(zd), C - 1, ptr(rd), ptr(ld_dev), ptr(loss), ptr(dz), ld_d, ptr(t), N, C, *setting,
                                                 1.0 / N, HF, stream()))


# ---- 2 / 3. fn_margin_weight_rnorm, fn_margin_wgrad_fix ----------------------------------------------------------------------
@pytest.mark.parametrize("C,E", [(37, 128), (1000, 512), (8, 8)])
def test_weight_rnorm_edges(lib, C, E):
    """Rows at scales 1e-2 .. 10, an all-zero row (the eps branch), a one-hot row (r == 1.0 bit for bit); nothing written beyond C."""
    w = mo.rnorm_inputs(C, E, seed=C)
    ref, bound = mo.rnorm_ref(w)
    wd = w.cuda()
    out = torch.full((C + 8,), 7.0, device="cuda")
    _lib.check(lib.fn_margin_weight_rnorm(ptr(wd), C, E, mo.EPS, ptr(out), stream()))
    torch.cuda.synchronize()
    eo.check_bound(out[:C], ref, bound, "rnorm")
    assert float(out[2]) == 1.0
    assert float(out[1]) == float(np.float32(1.0) / np.sqrt(np.float32(mo.EPS)))
    assert bool((out[C:] == 7.0).all())
    with pytest.raises(ValueError):
        _lib.check(lib.fn_margin_weight_rnorm(ptr(wd), C, E - 2, mo.EPS, ptr(out), stream()))


@pytest.mark.parametrize("C,E", [(37, 128), (1000, 512), (8, 8)])
def test_wgrad_fix_edges(lib, C, E):
    """dw -= r^2 t w on the rows below C only; t[0..C) zero afterwards, junk beyond intact."""
    rows = C + 3
    dw, w, rn, t = mo.wgrad_fix_inputs(C, E, seed=E, rows=rows)
    ref, bound = mo.wgrad_fix_ref(dw[:C], w[:C], rn, t)
    dwd, wd, rd = dw.cuda(), w.cuda(), rn.cuda()
    td = torch.full((C + 8,), JUNK, dtype=torch.int64, device="cuda")
    td[:C] = t.cuda()
    _lib.check(lib.fn_margin_wgrad_fix(ptr(dwd), ptr(wd), ptr(rd), ptr(td), C, E, stream()))
    torch.cuda.synchronize()
    eo.check_bound(dwd[:C], ref, bound, "corrected dw")
    assert float((dwd[:C].cpu() - dw[:C]).abs().max()) > 0
    assert torch.equal(dwd[C:].cpu(), dw[C:])
    assert int(td[:C].abs().max()) == 0 and bool((td[C:] == JUNK).all())


# ---- 4. one training step, stage by stage -----------------------------------------------------------------------------------
def _net(family, seed=0):
    if family == "v1":
        return Network(embedding_size=128, device="cuda:0", nrof_classes=NCLS, train_dtype=torch.float16, seed=seed)
    from facenet_amd.engine_v2 import NetworkV2
    return NetworkV2(128, config={"repeat": [2, 2, 2]}, device="cuda:0", nrof_classes=NCLS, seed=seed)


def _labels(N, seed):
    y = np.random.default_rng(seed).integers(0, NCLS, N)
    y[[0, 2, 3]] = 3                                                  # one class three times
    return y


def _fwd_bwd(tr):
    st = tr.net.stream()
    tr._zero()
    for ops in (tr.plan.fwd, tr.loss_ops, tr.plan.bwd):
        tr.plan.run_ops(ops, st)
    torch.cuda.synchronize()


@pytest.mark.parametrize("family", ["v1", "v2"])
def test_step_stage_by_stage(family):
    """Every stage of the head against fp64 on what the device produced for the stage before it, under that stage's derived bound:
    GEMM stages by the accumulation bound of tests/util.py (depth K, at most 16 partial sums), the others by margin_oracle /
    elementwise_oracle."""
    N, setting = 6, (64.0, 0.5, 0.0)
    net = _net(family)
    tr = Trainer(net, batch=N, loss="softmax", lr=0.01, margin_scale=setting[0], margin_arc=setting[1], margin_cos=setting[2])
    assert [op.name for op in tr.loss_ops] == MARGIN_OPS
    y = _labels(N, 5)
    tr.set_images(torch.from_numpy(structured_images(N, seed=11)), torch.from_numpy(y))
    L = net.layers["classifier/logits"]
    Cp, C, E, dt = L.cout, L.cout_real, net.E, tr.dt
    Gw = lambda: tr.G[L.w_off:L.w_off + L.numel].view(Cp, E).cpu().clone()
    st = net.stream()
    tr._zero()
    tr.plan.run_ops(tr.plan.fwd, st)
    snap = {}
    for op in tr.loss_ops:
        tr.plan.run_ops([op], st)
        torch.cuda.synchronize()
        if op.name == "margin_softmax":
            snap["t"] = tr.margin_t.cpu().clone()
        if op.name == "conv_wgrad:classifier":
            snap["G0"] = Gw()
    tr.plan.run_ops(tr.plan.bwd, st)
    torch.cuda.synchronize()
    emb, embn, emb_lp = tr.emb.cpu(), tr.embn.cpu(), tr.emb_lp.cpu()
    W = net.P[L.w_off:L.w_off + L.numel].view(Cp, E).cpu()
    W_lp = net.W_train[L.w_off:L.w_off + L.numel].view(Cp, E).cpu()
    rnorm, logits, dz = tr.rnorm.cpu(), tr.logits.cpu(), tr.dlogits.cpu()
    labels = torch.from_numpy(y).int()
    # the normalised embedding and its low-precision copy
    ref, bound, _, _ = eo.l2norm_ref(emb, 1e-10)
    eo.check_bound(embn, ref, bound, "embn")
    assert same_bits(emb_lp, embn.to(emb_lp.dtype))
    # reciprocal row norms of the fp32 master weights
    ref, bound = mo.rnorm_ref(W[:C])
    eo.check_bound(rnorm[:C], ref, bound, "rnorm")
    # logits = emb_lp . W_lp, no bias
    x64, w64 = emb_lp.double(), W_lp.double()
    assert_elementwise(logits, x64 @ w64.t(), x64.abs() @ w64.abs().t(), wgrad_k(E, 16), dt, "logits", out_f32=True)
    # loss, dz and t from the device's logits and rnorm
    o = mo.margin_ref(logits, rnorm, labels, C, *setting, 1.0 / N, dt)
    assert o["margin_ok"]
    eo.check_bound(tr.loss[0], o["loss"], o["e_loss"], "loss")
    assert tr.loss_value() == float(tr.loss[0]) and tr.loss_terms()["xent"] == tr.loss_value()
    eo.check_bound(dz[:, :C], o["dz"], o["e_dz"], "dz")
    assert float(dz[:, C:].float().abs().max()) == 0
    eo.check_bound(snap["t"][:C].double() * 2.0 ** -ACC_GRAD_BITS, o["t"], o["e_t"], "t")
    assert int(snap["t"][C:].abs().max()) == 0 and int(tr.margin_t.abs().max()) == 0        # left zeroed for the next step
    # the classifier's slice of G: dz^T emb_lp, then - r^2 t w on the rows below C
    d64 = dz.double()
    assert_elementwise(snap["G0"], d64.t() @ x64, d64.abs().t() @ x64.abs(), wgrad_k(N, 16), dt, "dW before the correction", out_f32=True)
    ref, bound = mo.wgrad_fix_ref(snap["G0"][:C], W[:C], rnorm[:C], snap["t"][:C])
    got = Gw()
    eo.check_bound(got[:C], ref, bound, "dW")
    assert float(got[C:].abs().max()) == 0                                                    # padded rows stay exactly zero
    assert float((got[:C] - snap["G0"][:C]).abs().max()) > 0
    # dembn = dz . W_lp, demb through the normalisation
    dembn = tr.dembn.cpu()
    assert_elementwise(dembn, d64 @ w64, d64.abs() @ w64.abs(), wgrad_k(Cp, 16), dt, "dembn", out_f32=True)
    ref, bound, ok = eo.l2norm_bwd_ref(emb, dembn, 1e-10)
    assert ok
    eo.check_bound(tr.demb.cpu(), ref, bound, "demb")
    # the bias is not read and gets a zero gradient
    assert float(tr.G[L.bias_off:L.bias_off + L.cout].abs().max()) == 0
    assert float(tr.G.abs().max()) > 0 and bool(torch.isfinite(tr.G).all())


# ---- 5. regularisers on top ----------------------------------------------------------------------------------------------------
def _within_one_ulp(got, want64):
    got = np.asarray(got, np.float32)
    return np.all(np.abs(got.astype(np.float64) - want64) <= np.spacing(np.abs(got)).astype(np.float64))


def test_regularizers_add_into_demb_after_the_normalisation_backward():
    N, cf, nf, p = 6, 0.5, 0.05, 1.0
    x = torch.from_numpy(structured_images(N, seed=11))
    y = _labels(N, 5)
    kw = dict(batch=N, loss="softmax", lr=0.01, margin_scale=30.0, margin_cos=0.35)
    tr0 = Trainer(_net("v1"), **kw)
    tr1 = Trainer(_net("v1"), center_factor=cf, prelogits_norm_factor=nf, prelogits_norm_p=p, **kw)
    assert [op.name for op in tr1.loss_ops] == MARGIN_OPS + ["center_loss"]
    centers = np.random.default_rng(1).standard_normal(tuple(tr1.centers.shape)).astype(np.float32)
    tr1.centers.copy_(torch.from_numpy(centers))
    for tr in (tr0, tr1):
        tr.set_images(x, torch.from_numpy(y))
        _fwd_bwd(tr)
    emb = tr1.emb.cpu().numpy()                                        # the regularisers act on the un-normalised embedding
    assert np.array_equal(emb, tr0.emb.cpu().numpy()) and tr0.loss_value() == tr1.loss_value()
    want = tr0.demb.cpu().numpy().astype(np.float64) + co.regularizer_grad(emb, y, centers, cf, nf, p)
    assert _within_one_ulp(tr1.demb.cpu().numpy(), want)
    assert float(np.abs(tr1.demb.cpu().numpy() - tr0.demb.cpu().numpy()).max()) > 0
    assert tr1.loss_terms()["xent"] == tr1.loss_value()


# ---- 6. reproducibility --------------------------------------------------------------------------------------------------------
def _run_steps(params, x, y, graph, steps=3):
    net = _net("v1", seed=3)
    net.load_keras_params(params)
    tr = Trainer(net, batch=len(y), loss="softmax", lr=0.01, margin_scale=64.0, margin_arc=0.5)
    tr.set_images(x, torch.from_numpy(y))
    if graph:
        tr.capture()
    embs = []
    for _ in range(steps):
        tr.step()
        torch.cuda.synchronize()
        embs.append(tr.emb.cpu().numpy().copy())
    assert np.isfinite(tr.loss_value())
    return embs + [net.P.cpu().numpy()]


def test_three_steps_eager_and_captured_are_bitwise_equal():
    x = torch.from_numpy(structured_images(6, seed=12))
    y = _labels(6, 8)
    params = _net("v1").export_keras_params()
    eager = _run_steps(params, x, y, graph=False)
    assert float(np.abs(eager[0] - eager[2]).max()) > 0               # the steps move the embedding
    for run in (_run_steps(params, x, y, graph=True), _run_steps(params, x, y, graph=True)):
        for a, b in zip(eager, run):
            assert np.array_equal(a, b)


# ---- 7. margin_scale = 0 -------------------------------------------------------------------------------------------------------
def test_margin_scale_zero_is_todays_trainer():
    x = torch.from_numpy(structured_images(4, seed=13))
    y = torch.tensor([1, 5, 5, 18])
    params = _net("v1").export_keras_params()
    trs = []
    for kw in ({}, dict(margin_scale=0.0, margin_arc=0.0, margin_cos=0.0)):
        net = _net("v1", seed=1)
        net.load_keras_params(params)
        tr = Trainer(net, batch=4, loss="softmax", lr=0.01, **kw)
        tr.set_images(x, y)
        tr.step()
        torch.cuda.synchronize()
        trs.append(tr)
    a, b = trs
    assert [op.name for op in a.step_ops] == [op.name for op in b.step_ops]
    assert not b.margin and not hasattr(b, "rnorm") and "margin_softmax" not in [op.name for op in b.step_ops]
    assert torch.equal(a.G, b.G) and torch.equal(a.net.P, b.net.P)


# ---- 8. two replicas -------------------------------------------------------------------------------------------------------------
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
        net = Network(embedding_size=128, device="cuda:0", nrof_classes=NCLS, train_dtype=torch.float16, seed=rank)
        tr = Trainer(net, batch=4, loss="softmax", lr=0.01, world_size=world, process_group=dist.group.WORLD, n_buckets=4,
                     margin_scale=64.0, margin_arc=0.5)
        y = np.array([[4, 7, 4, 0], [7, 4, 12, 4]][rank])
        tr.set_images(torch.from_numpy(structured_images(4, seed=50 + rank)), torch.from_numpy(y))
        if use_graph:
            tr.capture()
        for _ in range(2):
            tr.step()
        torch.cuda.synchronize()
        q.put((rank, net.P.cpu().numpy(), tr.loss_value()))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("use_graph", [False, True])
def test_two_replicas_keep_identical_parameters(use_graph):
    import torch.multiprocessing as mp
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_rank, args=(r, world, port, q, use_graph)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        res = sorted([q.get(timeout=300) for _ in range(world)], key=lambda t: t[0])
        for p in procs:
            p.join(timeout=60)                                          # every child under its own time limit
            assert p.exitcode == 0
    finally:
        for p in procs:
            if p.is_alive():
                p.kill()
    assert np.array_equal(res[0][1], res[1][1])                        # bitwise identical on both ranks
    assert np.isfinite(res[0][1]).all() and np.isfinite(res[0][2]) and np.isfinite(res[1][2])


# ---- 9. checkpoints --------------------------------------------------------------------------------------------------------------
def test_checkpoint_round_trip(tmp_path):
    x = torch.from_numpy(structured_images(4, seed=14))
    y = torch.tensor([2, 2, 9, 2])
    params = _net("v1").export_keras_params()

    def trainer(seed):
        net = _net("v1", seed=seed)
        net.load_keras_params(params)
        tr = Trainer(net, batch=4, loss="softmax", lr=0.01, margin_scale=30.0, margin_cos=0.35)
        tr.set_images(x, y)
        return tr

    tr = trainer(0)
    keys = set(tr.state_dict())
    tr.step()
    path = tmp_path / "ckpt.npz"
    tr.save_checkpoint(path, epoch=1)
    tr.step()
    torch.cuda.synchronize()
    with np.load(path) as z:
        assert set(z.files) == keys and not any("margin" in k for k in z.files)      # settings, not state
    tr2 = trainer(5)
    assert tr2.load_checkpoint(path) == 1
    tr2.step()
    torch.cuda.synchronize()
    a, b = tr.net.export_keras_params(), tr2.net.export_keras_params()
    for k in a:
        assert torch.equal(a[k], b[k]), k


# ---- 10. the app -----------------------------------------------------------------------------------------------------------------
def test_train_softmax_app_runs_the_margin_head():
    from facenet_amd.apps.train_softmax import train_softmax
    from facenet_amd.config import load_config
    logs = []
    cfg = load_config(overrides={"batch_size": 8, "loss": {"margin_scale": 30, "margin_cos": 0.35},
                                 "train": {"epoch": {"nrof_epochs": 2, "size": 4}, "learning_rate": {"value": 0.01}}})
    x = torch.from_numpy(structured_images(8, seed=4))
    y = torch.from_numpy(np.random.default_rng(5).integers(0, 37, 8))
    net, tr = train_softmax(cfg, 37, batches=((x, y) for _ in iter(int, 1)), embedding_size=128, log=logs.append)
    assert logs[0].startswith("margin softmax:") and "scale 30" in logs[0] and "cos 0.35" in logs[0]
    assert len(logs) == 3
    for line in logs[1:]:
        assert np.isfinite(float(line.split("  xent ")[1].split()[0]))
    names = [op.name for op in tr.step_ops]
    assert all(n in names for n in ("margin_rnorm", "margin_softmax", "margin_wgrad_fix")) and "softmax_xent" not in names
    assert tr.margin_scale == 30.0 and tr.margin_cos == 0.35 and tr.margin_arc == 0.0
