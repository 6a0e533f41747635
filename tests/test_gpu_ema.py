"""The moving average of the weights on the GPU (restated in tests/ema_oracle.py): the fused optimiser
entry through the C ABI, the shadow inside training steps of both model families, eager and captured, checkpoints, averaged
evaluation, data parallelism and the softmax app."""
import os
import socket

import numpy as np
import pytest
import torch

from facenet_amd import _lib
from facenet_amd.config import Config, load_config
from facenet_amd.engine import Network
from facenet_amd.train import Trainer
from tests import ema_oracle as eo
from tests.util import ptr, stream
from tests.util_data import structured_images

pytestmark = pytest.mark.gpu

NCLS, DECAY = 19, 0.9999
SWITCH = eo.switch_point(DECAY)


@pytest.fixture(autouse=True)
def _heuristic_tiles(monkeypatch):
    # trainers and models that are compared bit for bit run on the library's deterministic tile heuristic
    monkeypatch.setenv("FACENET_AUTOTUNE", "0")


# ---- 1. the kernel through ctypes --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [_lib.FN_BF16, _lib.FN_F16])
def test_fused_entry_matches_adam_and_the_oracle(dt):
    lib = _lib.load()
    n, n_lp, n_decay = 50_000, 30_000, 41_233
    rng = np.random.default_rng(dt)
    lp = torch.bfloat16 if dt == _lib.FN_BF16 else torch.float16
    w0 = rng.standard_normal(n).astype(np.float32)
    m0 = (rng.standard_normal(n) * 1e-2).astype(np.float32)
    v0 = (rng.random(n) * 1e-3).astype(np.float32)
    s0 = (w0 + rng.standard_normal(n) * 0.1).astype(np.float32)
    sentinel = np.float32(-1234.5)
    for t in (1, 2, 3, 1000, SWITCH - 1, SWITCH, SWITCH + 1, 10 ** 6):
        g = torch.from_numpy(rng.standard_normal(n).astype(np.float32)).cuda()
        bufs = []
        for fused in (False, True):
            w, m, v = (torch.from_numpy(a.copy()).cuda() for a in (w0, m0, v0))
            wlp = torch.zeros(n_lp + 8, dtype=lp, device="cuda")
            shadow = torch.from_numpy(np.concatenate([s0, np.full(4, sentinel, np.float32)])).cuda()
            hyper = torch.tensor([0.05, 1.0, 1.0, 0.5, 0.0, 0.0, 0.0, 0.0], device="cuda")
            hyper.view(torch.int32)[4:5].fill_(t - 1)
            _lib.check(lib.fn_adam_tick(ptr(hyper), 0.9, 0.999, stream()))
            args = (ptr(w), ptr(g), ptr(m), ptr(v), ptr(wlp), n_lp, n, n_decay, ptr(hyper), 0.9, 0.999, 0.1, 5e-4, dt)
            if fused:
                _lib.check(lib.fn_adam_keras_ema(*args, ptr(shadow), DECAY, stream()), "adam_keras_ema")
            else:
                _lib.check(lib.fn_adam_keras(*args, stream()), "adam_keras")
            torch.cuda.synchronize()
            assert hyper.view(torch.int32)[4].item() == t
            bufs.append([x.cpu() for x in (w, m, v, wlp, shadow)])
        (w, m, v, wlp, _), (wf, mf, vf, wlpf, s) = bufs
        for a, b in ((w, wf), (m, mf), (v, vf), (wlp.view(torch.int16), wlpf.view(torch.int16))):
            assert torch.equal(a, b), t
        want = eo.update(s0, wf.numpy(), t, DECAY)
        assert np.array_equal(s.numpy()[:n], want), t
        assert np.all(s.numpy()[n:] == sentinel)                    # nothing written past n
        assert not np.array_equal(want, s0)
    with pytest.raises(ValueError):
        _lib.check(lib.fn_adam_keras_ema(*args, ptr(shadow), 1.0, stream()), "adam_keras_ema")
    with pytest.raises(ValueError):
        _lib.check(lib.fn_adam_keras_ema(*args, None, DECAY, stream()), "adam_keras_ema")


# ---- 2. the shadow inside training steps -------------------------------------------------------------------------------------
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


def _trainer(family, loss, params, decay=DECAY, seed=1, **kw):
    net = _net(family, loss, seed=seed)
    net.load_keras_params(params)
    tr = Trainer(net, batch=6, loss=loss, lr=0.01, moving_average_decay=decay, **kw)
    x, y = _batch(loss)
    tr.set_images(x, y)
    return tr


def _trajectory(tr, steps, start_t=0):
    """Run `steps` steps; check the shadow against the oracle applied to the read-back P after each; return the states."""
    if start_t:
        tr.iterations = start_t
    s = None if tr.shadow is None else tr.shadow.cpu().numpy()
    out = []
    for k in range(steps):
        tr.step()
        torch.cuda.synchronize()
        P = tr.net.P.cpu().numpy()
        if s is not None:
            s = eo.update(s, P, start_t + k + 1, DECAY)
            assert np.array_equal(tr.shadow.cpu().numpy(), s), k
        out.append((P, tr.M.cpu().numpy(), tr.V.cpu().numpy(), tr.loss_value()))
    return out, s


@pytest.mark.parametrize("loss,start_t", [("triplet", 0), ("softmax", SWITCH - 3)])
def test_v1_shadow_follows_the_oracle_and_adam_is_unchanged(loss, start_t):
    params = _net("v1", loss).export_keras_params()
    on, off = _trainer("v1", loss, params), _trainer("v1", loss, params, decay=None)
    assert off.shadow is None and torch.equal(on.shadow, on.net.P)
    names_on, names_off = [op.name for op in on.step_ops], [op.name for op in off.step_ops]
    assert len(names_on) == len(names_off)
    assert [n for n in names_on if n != "adam_keras_ema"] == [n for n in names_off if n != "adam_keras"]
    s0 = on.shadow.cpu().numpy()
    a, s = _trajectory(on, 5, start_t)
    b, _ = _trajectory(off, 5, start_t)
    for (pa, ma, va, la), (pb, mb, vb, lb) in zip(a, b):
        assert np.array_equal(pa, pb) and np.array_equal(ma, mb) and np.array_equal(va, vb) and la == lb
    assert not np.array_equal(s, a[-1][0]) and not np.array_equal(s, s0)


def test_v2_shadow_follows_the_oracle():
    params = _net("v2", "softmax").export_keras_params()
    tr = _trainer("v2", "softmax", params)
    _trajectory(tr, 3)


def test_captured_steps_equal_eager_steps_and_capture_keeps_the_shadow():
    params = _net("v1", "softmax").export_keras_params()
    eager = _trainer("v1", "softmax", params)
    ref, _ = _trajectory(eager, 3)
    tr = _trainer("v1", "softmax", params)
    tr.shadow.mul_(0.5)                       # a shadow that is not P: capture() must leave it exactly as it is
    before = tr.shadow.clone()
    tr.capture()
    torch.cuda.synchronize()
    assert torch.equal(tr.shadow, before)
    tr.reset_average()
    got, _ = _trajectory(tr, 3)
    for (pa, ma, va, la), (pb, mb, vb, lb) in zip(ref, got):
        assert np.array_equal(pa, pb) and np.array_equal(ma, mb) and np.array_equal(va, vb) and la == lb
    assert torch.equal(tr.shadow, eager.shadow)


def test_invalid_decay_raises():
    net = _net("v1", "triplet")
    for bad in (-0.1, 1.0, 2.0):
        with pytest.raises(ValueError):
            Trainer(net, batch=6, loss="triplet", moving_average_decay=bad)
    tr = Trainer(net, batch=6, loss="triplet", moving_average_decay=0)
    assert tr.shadow is None
    with pytest.raises(RuntimeError):
        tr.reset_average()
    with pytest.raises(RuntimeError):
        tr.evaluate(np.zeros((2, 160, 160, 3), np.uint8), averaged=True)


# ---- 3. checkpoints ----------------------------------------------------------------------------------------------------------
def test_checkpoints(tmp_path):
    params = _net("v1", "softmax").export_keras_params()
    tr = _trainer("v1", "softmax", params)
    tr.step()
    tr.step()
    path = tmp_path / "ckpt.npz"
    tr.save_checkpoint(path, epoch=1)
    tr.step()
    torch.cuda.synchronize()
    with np.load(path) as z:
        keys = list(z.files)
    shadow_keys = [k for k in keys if k.endswith("/ExponentialMovingAverage:0")]
    n_trainable = len([1 for k, i in tr.net.variable_table() if not i.endswith(("moving_mean", "moving_variance"))])
    assert len(shadow_keys) == n_trainable
    # resume: bit-identical continuation
    tr2 = _trainer("v1", "softmax", _net("v1", "softmax", seed=5).export_keras_params(), seed=5)
    assert tr2.load_checkpoint(path) == 1
    tr2.step()
    torch.cuda.synchronize()
    for a, b in ((tr.net.P, tr2.net.P), (tr.shadow, tr2.shadow), (tr.M, tr2.M), (tr.V, tr2.V)):
        assert torch.equal(a, b)
    # a checkpoint without shadows starts the average at the loaded weights
    with np.load(path) as z:
        sd = {k: z[k] for k in z.files if k not in shadow_keys}
    old = tmp_path / "old.npz"
    np.savez(old, **sd)
    tr3 = _trainer("v1", "softmax", params, seed=6)
    tr3.shadow.fill_(3.0)
    tr3.load_checkpoint(old)
    assert torch.equal(tr3.shadow, tr3.net.P)
    # a plain trainer and load_keras_params ignore the shadow keys
    tr4 = _trainer("v1", "softmax", params, decay=None, seed=7)
    assert tr4.load_checkpoint(path) == 1
    assert torch.equal(tr4.net.P, tr3.net.P)
    assert not [k for k in tr4.state_dict() if "ExponentialMovingAverage" in k]
    net5 = _net("v1", "softmax", seed=8)
    with np.load(path) as z:
        net5.load_keras_params({k: torch.from_numpy(z[k]) for k in z.files})
    assert torch.equal(net5.P, tr3.net.P)


# ---- 4. averaged evaluation --------------------------------------------------------------------------------------------------
def test_averaged_evaluation_matches_the_saved_averaged_model(tmp_path):
    from facenet_amd.api import FaceNet
    params = _net("v1", "triplet").export_keras_params()
    tr = _trainer("v1", "triplet", params)
    for _ in range(3):
        tr.step()
    images = structured_images(8, seed=33)
    P = tr.net.P.clone()
    avg = tr.evaluate(images, averaged=True).cpu().numpy()
    torch.cuda.synchronize()
    assert torch.equal(tr.net.P, P) and not tr.net.folded_valid      # P restored bit for bit, the fold left to be redone
    raw = tr.evaluate(images).cpu().numpy()
    assert not np.array_equal(avg, raw)
    np.testing.assert_allclose(np.linalg.norm(avg, axis=1), 1.0, atol=1e-5)
    path = tmp_path / "averaged.npz"
    tr.save_averaged_weights(path)
    with np.load(path) as z:
        assert list(z.files) == list(tr.net.keras_variables().keys())
    model = FaceNet(Config({"path": str(path), "embedding_size": 128, "normalize": True}))
    assert np.array_equal(model.evaluate(images), avg)
    tr.save_checkpoint(tmp_path / "raw.npz")
    raw_model = FaceNet(Config({"path": str(tmp_path / "raw.npz"), "embedding_size": 128, "normalize": True}))
    assert np.array_equal(raw_model.evaluate(images), raw)


def test_averaged_evaluation_between_steps_leaves_training_unchanged():
    params = _net("v1", "softmax").export_keras_params()
    images = structured_images(4, seed=34)
    ref, _ = _trajectory(_trainer("v1", "softmax", params), 3)
    tr = _trainer("v1", "softmax", params)
    tr.capture()
    got = []
    for _ in range(3):
        tr.step()
        tr.evaluate(images, averaged=True)
        tr.evaluate(images)
        torch.cuda.synchronize()
        got.append((tr.net.P.cpu().numpy(), tr.M.cpu().numpy(), tr.V.cpu().numpy(), tr.loss_value()))
    for (pa, ma, va, la), (pb, mb, vb, lb) in zip(ref, got):
        assert np.array_equal(pa, pb) and np.array_equal(ma, mb) and np.array_equal(va, vb) and la == lb


# ---- 5. data parallelism -----------------------------------------------------------------------------------------------------
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
                     moving_average_decay=DECAY)
        tr.set_images(torch.from_numpy(structured_images(4, seed=60 + rank)), torch.tensor([[1, 5, 5, 18], [0, 3, 5, 9]][rank]))
        tr.capture()
        Ps, shadows = [net.P.cpu().numpy()], [tr.shadow.cpu().numpy()]
        for _ in range(2):
            tr.step()
            torch.cuda.synchronize()
            Ps.append(net.P.cpu().numpy())
            shadows.append(tr.shadow.cpu().numpy())
        n_avg = len(tr.averaged_variables())            # collective: both ranks call it
        q.put((rank, Ps, shadows, n_avg))
    finally:
        dist.destroy_process_group()


def test_two_replicas_keep_identical_shadows():
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
    (_, P0, S0, n0), (_, P1, S1, n1) = res
    assert n0 == n1 > 0
    assert np.array_equal(P0[0], P1[0]) and np.array_equal(S0[0], P0[0]) and np.array_equal(S1[0], P0[0])   # from the broadcast
    s = S0[0]
    for k in range(1, 3):
        assert np.array_equal(P0[k], P1[k]) and np.array_equal(S0[k], S1[k])
        s = eo.update(s, P0[k], k, DECAY)
        assert np.array_equal(S0[k], s)


# ---- 6. the softmax app ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("decay", [DECAY, None])
def test_train_softmax_app(tmp_path, decay):
    from facenet_amd.api import FaceNet
    from facenet_amd.apps.train_softmax import train_softmax
    model_dir = tmp_path / "run"
    train = {"epoch": {"nrof_epochs": 2, "size": 2}, "learning_rate": {"value": 0.01}}
    if decay is not None:
        train["moving_average_decay"] = decay
    cfg = load_config(overrides={"batch_size": 6, "train": train, "model": {"path": str(model_dir)}})
    x, y = _batch("softmax")
    net, tr = train_softmax(cfg, NCLS, batches=((x, y) for _ in iter(int, 1)), embedding_size=128, log=lambda *_: None)
    with np.load(model_dir / "run.npz") as z:
        keys = set(z.files)
    shadow_keys = {k for k in keys if k.endswith("/ExponentialMovingAverage:0")}
    plain = set(tr.net.keras_variables()) | {"epoch", "Adam/iter:0", "Adam/learning_rate:0"}
    if decay is None:
        assert tr.shadow is None and not shadow_keys and not (model_dir / "averaged").exists()
        assert keys == plain | {k for k in keys if k.startswith("Adam/")}
        return
    assert tr.iterations == 4 and keys - shadow_keys == plain | {k for k in keys if k.startswith("Adam/")}
    assert len(shadow_keys) == len([1 for k, i in tr.net.variable_table() if not i.endswith(("moving_mean", "moving_variance"))])
    assert [p.name for p in (model_dir / "averaged").iterdir()] == ["run.npz"]
    images = structured_images(4, seed=35)
    model = FaceNet(Config({"path": str(model_dir / "averaged"), "embedding_size": 128, "normalize": True}))
    assert np.array_equal(model.evaluate(images), tr.evaluate(images, averaged=True).cpu().numpy())
