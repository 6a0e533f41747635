"""The update rules of train.optimizer on the GPU (restated in tests/optimizer_oracle.py): the fused entry
through the C ABI, the rules inside training steps of both model families, eager and captured, checkpoints, data parallelism
and the training apps."""
import os
import socket
import warnings

import numpy as np
import pytest
import torch

from facenet_amd import _lib
from facenet_amd.config import load_config
from facenet_amd.engine import Network
from facenet_amd.train import OPTIMIZERS, Trainer
from tests import ema_oracle as eo
from tests import optimizer_oracle as oo
from tests.util import ptr, stream
from tests.util_data import structured_images

pytestmark = pytest.mark.gpu

NCLS, DECAY = 19, 0.9999
LRS = (0.01, 0.01, 0.004, 0.004, 0.001)         # a stepped schedule: the rules read lr from the device on every step


@pytest.fixture(autouse=True)
def _heuristic_tiles(monkeypatch):
    # trainers that are compared bit for bit run on the library's deterministic tile heuristic
    monkeypatch.setenv("FACENET_AUTOTUNE", "0")


# ---- 1. the kernel through ctypes --------------------------------------------------------------------------------------------
def _entry_args(rule, w, g, slots, wlp, n_lp, n, n_decay, hyper, dt, l2=5e-4):
    s2 = ptr(slots[1]) if len(slots) > 1 else None
    return (rule.code, ptr(w), ptr(g), ptr(slots[0]), s2, ptr(wlp), n_lp, n, n_decay, ptr(hyper), rule.rho, rule.momentum, rule.epsilon,
            l2, dt)


@pytest.mark.parametrize("dt", [_lib.FN_BF16, _lib.FN_F16])
@pytest.mark.parametrize("name", oo.RULES)
def test_fused_entry_matches_the_oracle(name, dt):
    lib, rule = _lib.load(), OPTIMIZERS[name]
    n, n_lp, n_decay, pad = 50_000, 30_000, 41_233, 8
    gs, l2 = 0.5, 5e-4
    rng = np.random.default_rng(10 * rule.code + dt)
    lp = torch.bfloat16 if dt == _lib.FN_BF16 else torch.float16
    sentinel = np.float32(-1234.5)
    w0 = rng.standard_normal(n).astype(np.float32)
    s0 = (w0 + rng.standard_normal(n) * 0.1).astype(np.float32)
    slots0 = oo.initial_slots(name, n)

    def dev(a):     # n values followed by `pad` sentinels: nothing may be written past n
        return torch.from_numpy(np.concatenate([a, np.full(pad, sentinel, np.float32)])).cuda()

    runs = []
    for fused in (False, True):
        w, shadow = dev(w0), dev(s0)
        slots = [dev(s) for s in slots0]
        wlp = torch.full((n_lp + pad,), -7.0, dtype=lp, device="cuda")
        hyper = torch.tensor([0.0, 1.0, 1.0, gs, 0.0, 0.0, 0.0, 0.0], device="cuda")
        runs.append((w, slots, wlp, hyper, shadow, fused))
    want_w, want_s, want_sh = w0, slots0, s0
    for k, lr in enumerate(LRS + (0.0005,)):
        G = (rng.standard_normal(n) * 0.1).astype(np.float32)
        g = torch.from_numpy(G).cuda()
        for w, slots, wlp, hyper, shadow, fused in runs:
            hyper[0:1].fill_(lr)
            _lib.check(lib.fn_adam_tick(ptr(hyper), 0.9, 0.999, stream()))
            args = _entry_args(rule, w, g, slots, wlp, n_lp, n, n_decay, hyper, dt, l2)
            if fused:
                _lib.check(lib.fn_opt_keras_ema(*args, ptr(shadow), DECAY, stream()), "opt_keras_ema")
            else:
                _lib.check(lib.fn_opt_keras(*args, stream()), "opt_keras")
        torch.cuda.synchronize()
        want_w, want_s = oo.step(name, want_w, G, want_s, lr, grad_scale=gs, l2=l2, n_decay=n_decay)
        want_sh = eo.update(want_sh, want_w, k + 1, DECAY)
        (w, slots, wlp, hyper, _, _), (wf, slotsf, wlpf, hyperf, shf, _) = runs
        assert hyper.view(torch.int32)[4].item() == hyperf.view(torch.int32)[4].item() == k + 1
        assert np.array_equal(w.cpu().numpy()[:n], want_w), k
        for a, b in zip(slots, want_s):
            assert np.array_equal(a.cpu().numpy()[:n], b), k
        pack = torch.from_numpy(want_w[:n_lp]).to(lp)                  # round to nearest even, as the Adam pack rounds
        assert torch.equal(wlp[:n_lp].cpu().view(torch.int16), pack.view(torch.int16)), k
        # the fused form: w, the slots and the pack bit-identical to the plain form, the shadow bit-exact against the oracle
        assert torch.equal(w, wf) and torch.equal(wlp.view(torch.int16), wlpf.view(torch.int16))
        assert all(torch.equal(a, b) for a, b in zip(slots, slotsf))
        assert np.array_equal(shf.cpu().numpy()[:n], want_sh), k
    for w, slots, wlp, _, shadow, _ in runs:
        for buf in [w, shadow] + slots:
            assert np.all(buf.cpu().numpy()[n:] == sentinel)
        assert np.all(wlp[n_lp:].float().cpu().numpy() == -7.0)
    assert not np.array_equal(want_w, w0) and not np.array_equal(want_sh, s0)


def test_bad_arguments_are_rejected():
    lib = _lib.load()
    n = 64
    w, g, s1, s2, shadow = (torch.zeros(n, device="cuda") for _ in range(5))
    wlp = torch.zeros(n, dtype=torch.bfloat16, device="cuda")
    hyper = torch.tensor([0.01, 1.0, 1.0, 1.0, 0.0, 0.0, 0.0, 0.0], device="cuda")
    rms = OPTIMIZERS["RMSPROP"]

    def call(code=rms.code, n=n, n_lp=n, n_decay=n, second=True, dt=_lib.FN_BF16, wp=True, ema=None):
        args = (code, ptr(w) if wp else None, ptr(g), ptr(s1), ptr(s2) if second else None, ptr(wlp), n_lp, n, n_decay, ptr(hyper),
                0.9, 0.9, 1.0, 5e-4, dt)
        if ema is None:
            return lib.fn_opt_keras(*args, stream())
        return lib.fn_opt_keras_ema(*args, ema[0], ema[1], stream())

    bad = [dict(n=62, n_lp=60, n_decay=60), dict(n_decay=n + 4), dict(n_decay=-1), dict(n_lp=n + 4), dict(n_lp=6), dict(second=False),
           dict(code=0), dict(code=5), dict(dt=7), dict(wp=False), dict(ema=(None, DECAY)), dict(ema=(ptr(shadow), 1.0)),
           dict(ema=(ptr(shadow), 0.0)), dict(code=OPTIMIZERS["ADADELTA"].code, second=False)]
    for kw in bad:
        with pytest.raises(ValueError):
            _lib.check(call(**kw), "opt_keras")
    torch.cuda.synchronize()
    assert not w.any() and not s1.any() and not s2.any() and not shadow.any()         # a rejected call launches nothing
    for code in (OPTIMIZERS["ADAGRAD"].code, OPTIMIZERS["MOM"].code):                  # one-slot rules need no second slot
        _lib.check(call(code=code, second=False), "opt_keras")
        _lib.check(call(code=code, second=False, ema=(ptr(shadow), DECAY)), "opt_keras_ema")
    torch.cuda.synchronize()


# ---- 2. the rules inside training steps --------------------------------------------------------------------------------------
def _net(family, loss, seed=0):
    ncls = NCLS if loss == "softmax" else None
    if family == "v1":
        return Network(embedding_size=128, device="cuda:0", nrof_classes=ncls, train_dtype=torch.float16, seed=seed)
    from facenet_amd.engine_v2 import NetworkV2
    return NetworkV2(128, config={"repeat": [2, 2, 2]}, device="cuda:0", nrof_classes=ncls, seed=seed)


def _batch(loss, N=6, seed=21):
    x = structured_images(N, seed=seed)
    if loss == "triplet":
        x[2], x[5] = x[1], x[4]             # the negative is the positive: every triplet violates the margin, the step has a gradient
        return torch.from_numpy(x), None
    return torch.from_numpy(x), torch.from_numpy(np.random.default_rng(seed).integers(0, NCLS, N))


def _trainer(family, loss, params, optimizer, seed=1, **kw):
    net = _net(family, loss, seed=seed)
    net.load_keras_params(params)
    tr = Trainer(net, batch=6, loss=loss, lr=0.01, optimizer=optimizer, **kw)
    x, y = _batch(loss)
    tr.set_images(x, y)
    return tr


def _state(tr):
    return [t.cpu().numpy().copy() for t in [tr.net.P] + tr.slots]


def _steps(tr, lrs=LRS, oracle=True):
    """One step per learning rate; with `oracle`, every step's P and slots must equal the oracle applied to the read-back G and
    the state before the step.  Returns [(P, slots..., loss)] per step."""
    n = tr.net.n_params
    out = []
    for lr in lrs:
        tr.set_learning_rate(lr)
        before, t = _state(tr), tr.iterations
        tr.step()
        torch.cuda.synchronize()
        after = _state(tr)
        assert tr.iterations == t + 1
        if oracle:
            G = tr.G.cpu().numpy()[:n]
            w, slots = oo.step(tr.optimizer, before[0][:n], G, [s[:n] for s in before[1:]], lr, grad_scale=1.0, l2=tr.l2,
                               n_decay=tr.net.n_decay)
            assert np.array_equal(after[0][:n], w) and np.array_equal(after[0][n:], before[0][n:])
            for a, b in zip(after[1:], slots):
                assert np.array_equal(a[:n], b)
            assert float(np.abs(G).max()) > 0
        out.append(after + [tr.loss_value()])
    return out


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        for u, v in zip(x[:-1], y[:-1]):
            assert np.array_equal(u, v)
        assert x[-1] == y[-1]


_ADAM_NAMES = {}


def _adam_launches(family, loss, params):
    if (family, loss) not in _ADAM_NAMES:
        _ADAM_NAMES[(family, loss)] = [op.name for op in _trainer(family, loss, params, "ADAM").step_ops]
    return _ADAM_NAMES[(family, loss)]


@pytest.mark.parametrize("loss", ["triplet", "softmax"])
@pytest.mark.parametrize("name", oo.RULES)
def test_v1_steps_follow_the_oracle_and_replay_equals_eager(name, loss):
    params = _net("v1", loss).export_keras_params()
    eager = _trainer("v1", loss, params, name)
    rule = OPTIMIZERS[name]
    assert eager.optimizer == name and eager.M is None and eager.V is None and len(eager.slots) == len(rule.slots)
    for buf, (_, init) in zip(eager.slots, rule.slots):
        assert torch.all(buf == init)
    names, adam = [op.name for op in eager.step_ops], _adam_launches("v1", loss, params)
    assert names.count(rule.op) == 1 and names.count("adam_tick") == 1
    assert [x if x != rule.op else "adam_keras" for x in names] == adam
    ref = _steps(eager)
    tr = _trainer("v1", loss, params, name)
    for buf in tr.slots:                       # state that is not the initial one: capture() must leave it exactly as it is
        buf.add_(0.25)
    tr.iterations = 7
    before = [t.clone() for t in [tr.net.P, tr.net.S_mean, tr.net.S_var, tr.hyper] + tr.slots]
    tr.capture()
    torch.cuda.synchronize()
    for a, b in zip(before, [tr.net.P, tr.net.S_mean, tr.net.S_var, tr.hyper] + tr.slots):
        assert torch.equal(a, b)
    tr.reset_optimizer()
    assert tr.iterations == 0 and all(torch.all(b == init) for b, (_, init) in zip(tr.slots, rule.slots))
    _same(ref, _steps(tr, oracle=False))


def test_v2_captured_equals_eager_and_dropout_follows_the_step_word():
    params = _net("v2", "softmax").export_keras_params()
    eager = _trainer("v2", "softmax", params, "RMSPROP")
    names = [op.name for op in eager.step_ops]
    assert [x if x != "rmsprop_keras" else "adam_keras" for x in names] == _adam_launches("v2", "softmax", params)
    ref, Ps, Gs = [], [], []
    for lr in LRS[:3]:
        Ps.append(eager.net.P.clone())
        ref += _steps(eager, (lr,))
        Gs.append(eager.G.clone())
    tr = _trainer("v2", "softmax", params, "RMSPROP")
    tr.capture()
    _same(ref, _steps(tr, LRS[:3], oracle=False))
    # an Adam trainer put at the RMSprop run's third step (same P, same `iterations`) draws the same dropout masks:
    # the forward and the gradients of that step are bit-identical
    adam = _trainer("v2", "softmax", params, "ADAM")
    adam.net.P.copy_(Ps[2])
    adam.net.folded_valid = False
    adam.net.refresh_packs()
    adam.iterations = 2
    adam.step()
    torch.cuda.synchronize()
    assert adam.iterations == 3 and adam.loss_value() == ref[2][-1] and torch.equal(adam.G, Gs[2])


def test_unknown_optimizer_raises():
    net = _net("v1", "triplet")
    for bad in ("SGD", "rmsprop", "NADAM", None):
        with pytest.raises(ValueError, match="Invalid optimization algorithm"):
            Trainer(net, batch=6, loss="triplet", optimizer=bad)


# ---- 3. checkpoints ----------------------------------------------------------------------------------------------------------
def _trainable(net):
    return [k for k, i in net.variable_table() if not i.endswith(("moving_mean", "moving_variance"))]


@pytest.mark.parametrize("name", oo.RULES)
def test_checkpoint_round_trip(tmp_path, name):
    rule = OPTIMIZERS[name]
    params = _net("v1", "softmax").export_keras_params()
    tr = _trainer("v1", "softmax", params, name, moving_average_decay=DECAY)
    _steps(tr, LRS[:2], oracle=False)
    path = tmp_path / "ckpt.npz"
    tr.save_checkpoint(path, epoch=1)
    with np.load(path) as z:
        keys = set(z.files)
        assert int(z[f"{rule.keras}/iter:0"]) == 2 and float(z[f"{rule.keras}/learning_rate:0"]) == np.float32(LRS[1])
    opt_keys = {k for k in keys if k.split("/")[0] in {r.keras for r in OPTIMIZERS.values()}}
    assert all(k.startswith(rule.keras + "/") for k in opt_keys)
    assert len(opt_keys) == len(rule.slots) * len(_trainable(tr.net)) + 2
    for slot, _ in rule.slots:
        assert f"{rule.keras}/inception_resnet_v1/block8_5/Conv2d_1x1/bias/{slot}:0" in keys
    cont = _steps(tr, LRS[2:], oracle=False)
    tr2 = _trainer("v1", "softmax", _net("v1", "softmax", seed=5).export_keras_params(), name, seed=5, moving_average_decay=DECAY)
    assert tr2.load_checkpoint(path) == 1 and tr2.iterations == 2
    _same(cont, _steps(tr2, LRS[2:], oracle=False))
    assert torch.equal(tr.shadow, tr2.shadow)


def test_checkpoint_of_another_optimizer_starts_the_optimizer_fresh(tmp_path):
    params = _net("v1", "softmax").export_keras_params()
    adam = _trainer("v1", "softmax", params, "ADAM")
    _steps(adam, LRS[:2], oracle=False)
    adam.save_checkpoint(tmp_path / "adam.npz", epoch=3)
    ada = _trainer("v1", "softmax", _net("v1", "softmax", seed=5).export_keras_params(), "ADAGRAD", seed=5)
    ada.set_learning_rate(0.02)
    _steps(ada, (0.02,), oracle=False)
    with pytest.warns(UserWarning, match="ADAM.*ADAGRAD"):
        assert ada.load_checkpoint(tmp_path / "adam.npz") == 3
    assert torch.equal(ada.net.P, adam.net.P) and ada.iterations == 0
    assert torch.all(ada.slots[0] == 0.1) and ada.hyper[0].item() == np.float32(0.02)
    ada.save_checkpoint(tmp_path / "adagrad.npz", epoch=4)
    with np.load(tmp_path / "adagrad.npz") as z:
        assert not [k for k in z.files if k.startswith("Adam/")] and int(z["Adagrad/iter:0"]) == 0
    adam2 = _trainer("v1", "softmax", params, "ADAM", seed=6)
    _steps(adam2, (0.01,), oracle=False)
    with pytest.warns(UserWarning, match="ADAGRAD.*ADAM"):
        assert adam2.load_checkpoint(tmp_path / "adagrad.npz") == 4
    assert torch.equal(adam2.net.P, adam.net.P) and adam2.iterations == 0 and not adam2.M.any() and not adam2.V.any()
    # an Adam checkpoint into an Adam trainer: restored, and silent
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert adam2.load_checkpoint(tmp_path / "adam.npz") == 3
    assert adam2.iterations == 2 and torch.equal(adam2.M, adam.M) and torch.equal(adam2.V, adam.V)


# ---- 4. data parallelism -----------------------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _rank(rank, world, port, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["FACENET_AUTOTUNE"] = "0"
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        net = Network(embedding_size=128, device="cuda:0", nrof_classes=NCLS, train_dtype=torch.float16, seed=rank)
        tr = Trainer(net, batch=4, loss="softmax", lr=0.01, world_size=world, process_group=dist.group.WORLD, n_buckets=4,
                     optimizer="RMSPROP")
        tr.set_images(torch.from_numpy(structured_images(4, seed=60 + rank)), torch.tensor([[1, 5, 5, 18], [0, 3, 5, 9]][rank]))
        tr.capture()
        states = [[t.cpu().numpy() for t in [net.P] + tr.slots]]
        for _ in range(2):
            tr.step()
            torch.cuda.synchronize()
            states.append([t.cpu().numpy() for t in [net.P] + tr.slots])
        q.put((rank, states, tr.iterations, [op.name for op in tr.step_ops].count("rmsprop_keras")))
    finally:
        dist.destroy_process_group()


def test_two_replicas_stay_identical():
    import torch.multiprocessing as mp
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_rank, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=600) for _ in range(world)], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    (_, s0, t0, k0), (_, s1, t1, k1) = res
    assert t0 == t1 == 2 and k0 == k1 == 1
    for a, b in zip(s0, s1):
        for u, v in zip(a, b):
            assert np.array_equal(u, v)
    assert not np.array_equal(s0[0][0], s0[-1][0]) and s0[-1][1].any()


# ---- 5. the training apps ----------------------------------------------------------------------------------------------------
def test_train_softmax_app_with_momentum(tmp_path):
    from facenet_amd.apps.train_softmax import train_softmax
    model_dir = tmp_path / "run"
    cfg = load_config(overrides={"batch_size": 6, "model": {"path": str(model_dir)},
                                 "train": {"optimizer": "MOM", "epoch": {"nrof_epochs": 2, "size": 2}, "learning_rate": {"value": 0.01}}})
    x, y = _batch("softmax")
    logs = []
    net, tr = train_softmax(cfg, NCLS, batches=((x, y) for _ in iter(int, 1)), embedding_size=128, log=logs.append)
    assert tr.optimizer == "MOM" and tr.iterations == 4
    assert logs[0] == "optimizer: MOM" and len(logs) == 3
    with np.load(model_dir / "run.npz") as z:
        keys = set(z.files)
        assert int(z["SGD/iter:0"]) == 4
    assert not [k for k in keys if k.startswith("Adam/")]
    sgd = {k for k in keys if k.startswith("SGD/")}
    assert {k for k in sgd if k.endswith("/momentum:0")} == sgd - {"SGD/iter:0", "SGD/learning_rate:0"}
    assert len(sgd) == len(_trainable(net)) + 2
    assert keys - sgd == set(net.keras_variables()) | {"epoch"}


def test_train_tripletloss_app_with_rmsprop():
    from facenet_amd.apps.train_tripletloss import train_tripletloss
    cfg = load_config(overrides={"train": {"optimizer": "RMSPROP", "epoch": {"nrof_epochs": 1, "size": 2},
                                           "learning_rate": {"value": 0.01}}})
    logs = []
    net, tr = train_tripletloss(cfg, people_per_batch=6, images_per_person=3, nrof_triplets=4, log=logs.append)
    assert tr.optimizer == "RMSPROP" and tr.iterations == 2 and np.isfinite(tr.loss_value())
    assert logs[0] == "optimizer: RMSPROP" and "triplet loss" in logs[-1] and len(logs) == 2
