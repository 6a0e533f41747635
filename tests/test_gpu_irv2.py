"""Inception-ResNet-v2 on the MI355X, through the C ABI: the two new kernels, inference and training steps against the fp32
restatement (tests/irv2_oracle.py), determinism / replay / checkpoints, and the app wiring.  (The 5x5 SAME convolution of
Mixed_5a: tests/test_gpu_conv.py CASES, element by element; every stage alone: tests/test_gpu_irv2_blocks.py.)

PARITY UNPINNED: the reference's v2 needs tf_slim; the restatement is this repo's, written from the topology table."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from facenet_amd import _lib
from facenet_amd.engine_v2 import NetworkV2
from facenet_amd.train import Trainer
from oracle import facenet_oracle as fo
from tests import irv2_oracle as ro
from tests.util import lp_dtype, ptr, rel_err, stream, structured_images

pytestmark = pytest.mark.gpu
DTS = [_lib.FN_F16, _lib.FN_BF16]
SMALL = {"repeat": [2, 2, 2]}
SMALL_RO = dict(ro.CFG, repeat=[2, 2, 2])


def _lp(shape, dt, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(lp_dtype(dt)).cuda()


# ---- AvgPool 3x3 / stride 1 / SAME ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("N, H, W, C, c0, ld", [(2, 17, 17, 192, 0, 192), (3, 7, 5, 24, 8, 48), (1, 1, 1, 8, 0, 8), (2, 2, 9, 16, 16, 40)])
def test_avgpool3x3s1(lib, dt, N, H, W, C, c0, ld):
    x = _lp((N, H, W, ld), dt, 1)
    y = torch.full((N, H, W, ld), 7.0, dtype=lp_dtype(dt), device="cuda")
    _lib.check(lib.fn_avgpool3x3s1_fwd(ptr(x, c0), ld, ptr(y, c0), ld, N, H, W, C, dt, stream()))
    xr = x[..., c0:c0 + C].float().cpu().permute(0, 3, 1, 2).requires_grad_(True)
    yr = F.avg_pool2d(xr, 3, 1, 1, count_include_pad=False)
    torch.cuda.synchronize()
    tol = 1e-2 if dt == _lib.FN_BF16 else 2e-3
    assert rel_err(y[..., c0:c0 + C], yr.detach().permute(0, 2, 3, 1)) < tol
    assert (y[..., :c0].float() == 7).all() and (y[..., c0 + C:].float() == 7).all()       # outside the slice untouched
    dy = _lp((N, H, W, ld), dt, 2)
    yr.backward(dy[..., c0:c0 + C].float().cpu().permute(0, 3, 1, 2))
    ref = xr.grad.permute(0, 2, 3, 1)
    dx = torch.full((N, H, W, ld), 7.0, dtype=lp_dtype(dt), device="cuda")
    _lib.check(lib.fn_avgpool3x3s1_bwd(ptr(dy, c0), ld, ptr(dx, c0), ld, N, H, W, C, 0, dt, stream()))
    torch.cuda.synchronize()
    assert rel_err(dx[..., c0:c0 + C], ref) < tol
    assert (dx[..., :c0].float() == 7).all() and (dx[..., c0 + C:].float() == 7).all()
    base = dx.clone()
    _lib.check(lib.fn_avgpool3x3s1_bwd(ptr(dy, c0), ld, ptr(dx, c0), ld, N, H, W, C, 1, dt, stream()))    # accumulate
    torch.cuda.synchronize()
    assert rel_err(dx[..., c0:c0 + C], base[..., c0:c0 + C].float().cpu() + ref) < tol


# ---- dropout -------------------------------------------------------------------------------------------------------------
def _dropout(lib, x, keep, seed, rank, step, dt, bwd=False):
    y = torch.empty_like(x)
    fn = lib.fn_dropout_bwd if bwd else lib.fn_dropout_fwd
    _lib.check(fn(ptr(x), ptr(y), x.shape[0], x.shape[1], keep, seed, rank, ptr(step), dt, stream()))
    return y


@pytest.mark.parametrize("dt", DTS)
def test_dropout_mask_matches_numpy_hash(lib, dt):
    N, Cc, keep = 24, 1536, 0.5
    x = torch.ones(N, Cc, dtype=lp_dtype(dt), device="cuda")
    step = torch.tensor([5], dtype=torch.int32, device="cuda")
    y = _dropout(lib, x, keep, 7, 1, step, dt).float().cpu()
    mask = ro.dropout_mask(7, 1, 5, N, Cc, keep)
    assert torch.equal(y != 0, torch.from_numpy(mask))
    assert (y[y != 0] == 2.0).all()
    assert abs(mask.mean() - keep) < 0.01
    for keep2 in (0.8, 0.1):
        y2 = _dropout(lib, x, keep2, 7, 1, step, dt).float().cpu()
        assert torch.equal(y2 != 0, torch.from_numpy(ro.dropout_mask(7, 1, 5, N, Cc, keep2)))
    # a new step and another rank draw other masks
    step6 = torch.tensor([6], dtype=torch.int32, device="cuda")
    assert not torch.equal(_dropout(lib, x, keep, 7, 1, step6, dt).float().cpu() != 0, y != 0)
    assert not torch.equal(_dropout(lib, x, keep, 7, 0, step, dt).float().cpu() != 0, y != 0)
    # backward applies the forward's mask and scale
    g = _lp((N, Cc), dt, 3)
    dx = _dropout(lib, g, keep, 7, 1, step, dt, bwd=True).float().cpu()
    assert torch.equal(dx, (g.float().cpu() * torch.from_numpy(mask) * 2.0).to(lp_dtype(dt)).float())


def test_dropout_graph_replay_matches_eager(lib):
    dt, N, Cc = _lib.FN_BF16, 9, 1536
    x = _lp((N, Cc), dt, 4)
    step = torch.tensor([0], dtype=torch.int32, device="cuda")
    y = torch.empty_like(x)
    run = lambda: _lib.check(lib.fn_dropout_fwd(ptr(x), ptr(y), N, Cc, 0.5, 3, 0, ptr(step), dt,
                                                torch.cuda.current_stream().cuda_stream))
    run()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run()
    for t in (0, 1, 2):
        step.fill_(t)
        g.replay()
        torch.cuda.synchronize()
        replayed = y.clone()
        run()
        torch.cuda.synchronize()
        assert torch.equal(replayed, y), t
        assert torch.equal(y.float().cpu() != 0, torch.from_numpy(ro.dropout_mask(3, 0, t, N, Cc, 0.5)) & (x.float().cpu() != 0))


# ---- inference -----------------------------------------------------------------------------------------------------------
def _perturbed(net, seed=1):
    p = net.export_keras_params()
    g = torch.Generator().manual_seed(seed)
    for k in p:
        if k.endswith("moving_mean"):
            p[k] = torch.randn(p[k].shape, generator=g) * 0.1
        elif k.endswith("moving_variance"):
            p[k] = 0.5 + torch.rand(p[k].shape, generator=g)
        elif k.endswith("beta"):
            p[k] = torch.randn(p[k].shape, generator=g) * 0.1
    net.load_keras_params(p)
    return p


@pytest.mark.parametrize("E", [128, 512])
def test_inference_embeddings(E):
    """16 images, unit-norm embeddings against the fp32 restatement: f16 row L2 error <= 1e-3, bf16 <= 2e-2
    (the bounds of the v1 test, tests/test_gpu_model.py)."""
    from facenet_amd.config import Config
    from facenet_amd.models.inception_resnet_v2 import InceptionResnetV2, default_model_config
    x = np.random.default_rng(0).integers(0, 256, (16, 160, 160, 3), dtype=np.uint8)
    cfg = dict(default_model_config.as_dict, embedding_size=E)
    params = None
    for dt, tol in ((torch.float16, 1e-3), (torch.bfloat16, 2e-2)):
        model = InceptionResnetV2((160, 160, 3), None, Config(cfg), device="cuda:0", infer_dtype=dt)
        params = params or _perturbed(model.network)
        model.network.load_keras_params(params)
        if dt == torch.float16:
            ref = fo.l2_normalize(ro.IRv2(params).forward(x, training=False))
        emb = model(torch.from_numpy(x), training=False).cpu()
        err = (emb - ref).norm(dim=1).max().item()
        print(f"v2 E={E} {dt}: max row L2 err {err:.3e}")
        assert err <= tol
        assert torch.allclose(emb.norm(dim=1), torch.ones(16), atol=1e-5)
        assert emb.shape == (16, E)


def test_inference_299_and_end_points():
    from facenet_amd.models.inception_resnet_v2 import inference
    x = torch.from_numpy(np.random.default_rng(1).integers(0, 256, (3, 299, 299, 3), dtype=np.uint8))
    emb, ep = inference(x, phase_train=False, device="cuda:0")
    assert emb.shape == (3, 512) and torch.isfinite(emb).all()
    assert ep["Mixed_5a"].shape == (3, 35, 35, 320) and ep["Mixed_6a"].shape == (3, 17, 17, 1088)
    assert ep["Mixed_7a"].shape == (3, 8, 8, 2080) and ep["Conv2d_7b_1x1"].shape == (3, 8, 8, 1536)
    assert ep["PreLogitsFlatten"].shape == (3, 1536)
    # 299x299x3 uint8 images are not 16-byte multiples: the normaliser's unaligned head / tail path (facenet.py:72-77)
    from facenet_amd.models import inception_resnet_v2 as m2
    model = next(v for k, v in m2._models.items() if k[1] == 299)
    got = model._plan(3, False).bufs["input"].act[..., :3].float().cpu()
    assert (got - fo.image_processing(x.numpy(), 0, 299)).abs().max().item() < 2e-3


# ---- training steps --------------------------------------------------------------------------------------------------------
def _rel(a, b):
    return (a - b).norm().item() / (b.norm().item() + 1e-12)


def _train_once(loss, dt, keep, N, ncls=None, labels=None, x=None):
    net = NetworkV2(128, config=dict(SMALL, keep_probability=keep), device="cuda:0", train_dtype=dt, nrof_classes=ncls)
    params = net.export_keras_params()
    tr = Trainer(net, batch=N, loss=loss, alpha=0.2, l2=0.0)
    tr.set_images(torch.from_numpy(x), torch.from_numpy(labels) if labels is not None else None)
    st = net.stream()
    tr._zero()
    for ops in (tr.plan.fwd, tr.loss_ops, tr.plan.bwd):
        tr.plan.run_ops(ops, st)
    torch.cuda.synchronize()
    return net, tr, params


@pytest.mark.parametrize("keep", [1.0, 0.5])
@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("loss", ["triplet", "softmax"])
def test_train_step_gradients(loss, dt, keep):
    """Loss, train-mode embedding and gradients against autograd on the restatement (repeat [2,2,2]); the HIP error stays within
    1.25x (+ slack) of what storage rounding alone costs (the bounds of tests/test_gpu_model.py).  keep 0.5 uses the hash mask."""
    N = 9 if loss == "triplet" else 8
    ncls, labels = (37, np.random.default_rng(5).integers(0, 37, N)) if loss == "softmax" else (None, None)
    x = structured_images(N, seed=3)
    net, tr, params = _train_once(loss, dt, keep, N, ncls, labels, x)
    masks = ro.dropout_mask(0, 0, 0, N, 1536, keep) if keep < 1 else None
    loss32, g32, emb32, stats32 = ro.train_step_grads(params, x, loss, None, keep, masks, labels, cfg=SMALL_RO)
    lossq, gq, embq, _ = ro.train_step_grads(params, x, loss, dt, keep, masks, labels, cfg=SMALL_RO)
    emb = tr.emb.float().cpu()
    f16 = dt == torch.float16
    print(f"{loss} {dt} keep {keep}: emb rel err {_rel(emb, emb32):.3e} (rounding {_rel(embq, emb32):.3e}); "
          f"loss {tr.loss_value():.5f} fp32 {loss32:.5f} rounding {lossq:.5f}")
    assert _rel(emb, emb32) < 1.25 * _rel(embq, emb32) + 5e-3
    assert abs(tr.loss_value() - loss32) < (2e-2 if f16 else 8e-2)
    mine = net.export_keras_grads(tr.G)
    keys = [k for k, g in g32.items() if g.norm().item() > 1e-4]
    e32 = np.array([_rel(mine[k], g32[k]) for k in keys])
    eq = np.array([_rel(gq[k], g32[k]) for k in keys])
    flat = lambda d: torch.cat([d[k].reshape(-1) for k in keys])
    cos = F.cosine_similarity(flat(mine), flat(g32), dim=0).item()
    print(f"  grads: median rel err HIP-fp32 {np.median(e32):.3f} rounding-fp32 {np.median(eq):.3f}; max {e32.max():.3f}/{eq.max():.3f}; "
          f"cosine {cos:.4f}")
    assert np.median(e32) < 1.25 * np.median(eq) + 0.02
    assert e32.max() < 1.25 * eq.max() + 0.05
    assert cos > (0.98 if f16 else 0.88)
    # moving statistics follow momentum 0.995 (0.99 would move them twice as far from the initial (0, 1))
    stats = net.export_keras_params()
    for k in ("Conv2d_1a_3x3/bn/moving_mean", "Mixed_5a/Branch_3/Conv2d_0b_1x1/bn/moving_variance",
              "Repeat_1/block17_2/Branch_1/Conv2d_0b_1x7/bn/moving_mean", "Bottleneck/bn/moving_mean"):
        assert torch.allclose(stats[k], stats32[k], rtol=3e-2, atol=3e-4), k


# ---- determinism, replay, checkpoints ------------------------------------------------------------------------------------
def _trainer(seed=0):
    net = NetworkV2(128, config=SMALL, device="cuda:0", seed=seed)
    tr = Trainer(net, batch=9, loss="triplet", alpha=0.2)
    xt = structured_images(9, seed=3)
    xt[2], xt[5] = xt[1], xt[4]            # every triplet violates the margin: a real gradient every step
    tr.set_images(torch.from_numpy(xt))
    return net, tr


def _state(net, tr):
    torch.cuda.synchronize()
    return [t.clone() for t in (net.P, net.S_mean, net.S_var, tr.M, tr.V, tr.emb)]


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def test_captured_steps_deterministic_and_equal_eager(tmp_path):
    runs = []
    for _ in range(2):
        net, tr = _trainer()
        tr.capture()
        for _ in range(3):
            tr.step()
        runs.append(_state(net, tr))
    assert _same(runs[0], runs[1])
    net, tr = _trainer()
    for _ in range(3):
        tr.step_eager()
    assert _same(_state(net, tr), runs[0])
    # checkpoint after 2 steps -> fresh trainer -> 1 more step equals 3 uninterrupted steps (dropout masks included: the step
    # word is Adam's iterations, restored by the checkpoint)
    net, tr = _trainer()
    tr.capture()
    tr.step()
    tr.step()
    tr.save_checkpoint(tmp_path / "v2.npz", epoch=1)
    z = np.load(tmp_path / "v2.npz")
    assert "InceptionResnetV2/Mixed_5a/Branch_1/Conv2d_0b_5x5/weights" in z.files
    assert "Adam/InceptionResnetV2/Bottleneck/weights/m:0" in z.files and int(z["Adam/iter:0"]) == 2
    net2, tr2 = _trainer()
    assert tr2.load_checkpoint(tmp_path / "v2.npz") == 1
    net2.refresh_packs()
    tr2.capture()
    tr2.step()
    assert _same(_state(net2, tr2), runs[0])


def test_model_training_call_owns_its_step():
    """model(x, training=True) without a Trainer: the plan's own counter advances the dropout mask call by call."""
    from facenet_amd.models.inception_resnet_v2 import InceptionResnetV2
    from facenet_amd.config import Config
    model = InceptionResnetV2((160, 160, 3), None, Config(dict(SMALL, embedding_size=128)), device="cuda:0")
    x = torch.from_numpy(structured_images(6, seed=2))
    p = model.network.export_keras_params()
    a = model(x, training=True).cpu()
    model.network.load_keras_params(p)          # undo the moving-statistics update
    b = model(x, training=True).cpu()
    assert not torch.equal(a, b)
    plan = model._plans[(6, True)]
    assert int(plan.step_word.item()) == 2


# ---- app -----------------------------------------------------------------------------------------------------------------
def test_train_softmax_app_v2_learns():
    from facenet_amd.apps.train_softmax import train_softmax
    from facenet_amd.config import load_config
    logs = []
    cfg = load_config(overrides={"batch_size": 8, "model": {"module": "facenet.models.inception_resnet_v2", "config": SMALL},
                                 "train": {"epoch": {"nrof_epochs": 2, "size": 4}, "learning_rate": {"value": 0.01}}})
    x = torch.from_numpy(structured_images(8, seed=4))
    y = torch.from_numpy(np.random.default_rng(5).integers(0, 37, 8))
    net, tr = train_softmax(cfg, 37, batches=((x, y) for _ in iter(int, 1)), embedding_size=128, log=logs.append)
    assert isinstance(net, NetworkV2) and len(logs) == 2
    first = float(logs[0].split("xent ")[1].split()[0])
    last = tr.loss_value()
    print(logs)
    assert np.isfinite(last) and last < first
