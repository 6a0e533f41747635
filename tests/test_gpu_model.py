"""End-to-end parity of the HIP path against the CPU fp32 oracle (oracle/facenet_oracle.py).

PARITY UNPINNED by the reference (it ships no vectors): the oracle is this repo's restatement."""
import numpy as np
import pytest
import torch

from facenet_amd.engine import Network
from facenet_amd.train import Trainer
from oracle import facenet_oracle as fo

pytestmark = pytest.mark.gpu


def _images(n, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (n, 160, 160, 3), dtype=np.uint8)


@pytest.fixture(scope="module")
def net128():
    net = Network(embedding_size=128, device="cuda:0")
    return net


def test_variable_counts(net128):
    assert net128.count_variables() == (22808144, 22779312)      # SURVEY.md shape table, E=128


def test_init_matches_oracle_declaration_order(net128):
    params, _, _ = fo.build_params(128, seed=0)
    mine = net128.init_keras_params(0)
    assert list(mine.keys()) == list(params.keys())
    for k in params:
        assert torch.equal(mine[k], params[k]), k


@pytest.mark.parametrize("variant", ["fresh", "perturbed"])
@pytest.mark.parametrize("E", [128, 512])
def test_forward_embeddings_c1(variant, E):
    """BASELINE.json configs[0] / SURVEY.md 8d C1: 16 random uint8 images, unit-norm embeddings, max row L2 error
    <= 1e-3 (f16 storage, fp32 accumulate).  bf16 storage is reported against its own looser bound (2e-2)."""
    params, _, _ = fo.build_params(E, seed=0)
    if variant == "perturbed":
        fo.perturb_bn_stats(params, seed=1)
    x = _images(16)
    ref = fo.Oracle(params).forward(x, training=False)
    for dt, tol in ((torch.float16, 1e-3), (torch.bfloat16, 2e-2)):
        net = Network(embedding_size=E, device="cuda:0", infer_dtype=dt)
        net.load_keras_params(params)
        plan = net.plan(16, training=False)
        plan.images.copy_(torch.from_numpy(x))
        plan.run_forward()
        torch.cuda.synchronize()
        emb = fo.l2_normalize(plan.embedding.buf.act.view(16, E).float().cpu())
        err = (emb - ref).norm(dim=1).max().item()
        print(f"C1 {variant} E={E} {dt}: max row L2 err {err:.3e}")
        assert err <= tol
        assert torch.allclose(emb.norm(dim=1), torch.ones(16), atol=1e-5)


def _rel(a, b):
    return (a - b).norm().item() / (b.norm().item() + 1e-12)


def _grad_report(net, G, g32, gq):
    """Per-parameter relative errors: HIP vs fp32 oracle, HIP vs storage-rounding oracle, rounding oracle vs fp32."""
    mine = net.export_keras_grads(G)
    keys = [k for k, g in g32.items() if g.norm().item() > 1e-4]
    e_hip32 = np.array([_rel(mine[k], g32[k]) for k in keys])
    e_hipq = np.array([_rel(mine[k], gq[k]) for k in keys])
    e_q32 = np.array([_rel(gq[k], g32[k]) for k in keys])
    flat = lambda d: torch.cat([d[k].reshape(-1) for k in keys])
    cos = torch.nn.functional.cosine_similarity(flat(mine), flat(g32), dim=0).item()
    return mine, keys, e_hip32, e_hipq, e_q32, cos


def _train_once(params, x, loss, dt, **kw):
    E = params["features/logits/kernel"].shape[1]
    ncls = params["classifier/logits/kernel"].shape[1] if "classifier/logits/kernel" in params else None
    net = Network(embedding_size=E, device="cuda:0", train_dtype=dt, nrof_classes=ncls)
    net.load_keras_params(params)
    tr = Trainer(net, batch=x.shape[0], loss=loss, alpha=0.2, l2=0.0)
    tr.set_images(torch.from_numpy(x), torch.from_numpy(kw["labels"]) if "labels" in kw else None)
    st = net.stream()
    tr._zero()
    tr.plan.run_ops(tr.plan.fwd, st)
    tr.plan.run_ops(tr.loss_ops, st)
    tr.plan.run_ops(tr.plan.bwd, st)
    torch.cuda.synchronize()
    return net, tr


# Gradients of a freshly initialised BatchNorm network at batch 9 are ill-conditioned: rounding activations to
# f16 / bf16 alone (tests/quant_oracle.py, everything else fp32 autograd) moves them by ~15 % / ~40 % relative to
# fp32, because each small-batch BN backward projects most of the incoming gradient away.  The bar is therefore:
# the HIP path must be as close to the fp32 oracle as that ideal low-precision-storage model is (x1.25 + 0.02),
# closer to the rounding model than the rounding model is to fp32, and tight where no BN backward intervenes.
@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
def test_triplet_train_step_gradients(dt):
    """forward(training=True) + l2_normalize + triplet loss + backward vs autograd on the oracle (batch 9 = 3 triplets)."""
    from tests.quant_oracle import quant_train_step_grads
    from tests.util import structured_images
    E, N = 128, 9
    params, trainable, _ = fo.build_params(E, seed=0)
    x = structured_images(N, seed=3)
    loss_ref, _, g32, new_stats, emb_ref = fo.train_step_grads(params, trainable, [], x, "triplet", alpha=0.2)
    loss_q, gq, emb_q = quant_train_step_grads(params, trainable, x, "triplet", dt)
    net, tr = _train_once(params, x, "triplet", dt)
    emb = tr.emb.float().cpu()
    f16 = dt == torch.float16
    print(f"{dt}: train-mode embedding rel err vs fp32 {_rel(emb, emb_ref):.3e} (rounding model {_rel(emb_q, emb_ref):.3e}); "
          f"loss {tr.loss_value():.5f} fp32 {loss_ref:.5f} rounding {loss_q:.5f}")
    assert _rel(emb, emb_ref) < 1.25 * _rel(emb_q, emb_ref) + 5e-3
    assert abs(tr.loss_value() - loss_ref) < (1e-2 if f16 else 5e-2)
    mine, keys, e_hip32, e_hipq, e_q32, cos = _grad_report(net, tr.G, g32, gq)
    print(f"  grads: median rel err HIP-fp32 {np.median(e_hip32):.3f}  HIP-rounding {np.median(e_hipq):.3f}  rounding-fp32 {np.median(e_q32):.3f}; "
          f"max {e_hip32.max():.3f}/{e_q32.max():.3f}; cosine {cos:.4f}")
    assert np.median(e_hip32) < 1.25 * np.median(e_q32) + 0.02
    assert e_hip32.max() < 1.25 * e_q32.max() + 0.05
    assert np.median(e_hipq) < np.median(e_q32)
    assert cos > (0.98 if f16 else 0.88)
    # no BatchNorm backward between the loss and these two: tight
    for k in ("features/logits/kernel", "block8_2/up/kernel"):
        assert _rel(mine[k], g32[k]) < (0.03 if f16 else 0.2), k
    # moving statistics follow momentum 0.99 with the biased batch variance (SURVEY.md hazard 3)
    stats = net.export_keras_params()
    for k in ("conv2d/Conv2d_1a_3x3/bn/moving_mean", "block17/3/tower_conv1/Conv2d_0b_1x7/bn/moving_variance", "features/bn/moving_mean"):
        assert torch.allclose(stats[k], new_stats[k], rtol=3e-2, atol=3e-3), k


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
def test_softmax_train_step_gradients(dt):
    """apps/train_softmax.py:49-104 step: classifier Dense + sparse softmax cross-entropy (batch 8, 37 classes)."""
    from tests.quant_oracle import quant_train_step_grads
    from tests.util import structured_images
    E, N, Cc = 128, 8, 37
    params, trainable, _ = fo.build_params(E, seed=0, nrof_classes=Cc)
    x = structured_images(N, seed=4)
    labels = np.random.default_rng(5).integers(0, Cc, N)
    loss_ref, _, g32, _, _ = fo.train_step_grads(params, trainable, [], x, "softmax", labels=labels)
    loss_q, gq, _ = quant_train_step_grads(params, trainable, x, "softmax", dt, labels=labels)
    net, tr = _train_once(params, x, "softmax", dt, labels=labels)
    f16 = dt == torch.float16
    print(f"{dt}: softmax loss {tr.loss_value():.5f} fp32 {loss_ref:.5f} rounding {loss_q:.5f}")
    assert abs(tr.loss_value() - loss_ref) < (2e-2 if f16 else 8e-2)
    mine, keys, e_hip32, e_hipq, e_q32, cos = _grad_report(net, tr.G, g32, gq)
    print(f"  grads: median rel err HIP-fp32 {np.median(e_hip32):.3f}  HIP-rounding {np.median(e_hipq):.3f}  rounding-fp32 {np.median(e_q32):.3f}; cosine {cos:.4f}")
    assert np.median(e_hip32) < 1.25 * np.median(e_q32) + 0.02
    assert e_hip32.max() < 1.25 * e_q32.max() + 0.05
    assert np.median(e_hipq) < np.median(e_q32)
    assert cos > (0.98 if f16 else 0.88)
    for k in ("classifier/logits/kernel", "classifier/logits/bias"):
        assert _rel(mine[k], g32[k]) < (0.02 if f16 else 0.08), k


def test_scheduled_multistream_step_matches_serial_replay():
    """The dependency scheduler (2 streams, eager and captured into a HIP graph) must reproduce the single-stream program-order
    replay of a full optimiser step.  Training is reproducible bit for bit (no floating-point atomics: fixed-point statistics and
    bias gradients, slab-reduced weight gradients), so every mode -- and a second serial run -- gives IDENTICAL loss, embeddings,
    gradients and parameters."""
    from tests.util import structured_images
    E, N = 128, 6
    params, _, _ = fo.build_params(E, seed=0)
    x = torch.from_numpy(structured_images(N, seed=7))
    results = []
    for mode in ("serial", "serial", "streams", "graph"):
        net = Network(embedding_size=E, device="cuda:0", train_dtype=torch.float16)
        net.load_keras_params(params)
        tr = Trainer(net, batch=N, loss="triplet", alpha=0.2, lr=0.01, n_streams=2)
        tr.set_images(x)
        if mode == "serial":
            tr.plan.run_ops(tr.step_ops, net.stream())       # the step's launches in program order on ONE stream
        elif mode == "streams":
            tr.step_eager()
        else:
            tr.capture()                     # side-effect free: its warm-up step is undone
            tr.step()
        torch.cuda.synchronize()
        results.append((tr.loss_value(), tr.emb.clone(), tr.G.clone(), net.P.clone()))
        st_ = tr.segments[0][0].stats()
        assert st_["stream1"] > 0                            # the placement really is multi-stream
    assert float(results[0][2].abs().max()) > 0 and float((results[0][3] - net.P).abs().max()) == 0
    for r, name in zip(results[1:], ("serial again", "streams", "graph")):
        assert r[0] == results[0][0], name
        for a, b in zip(r[1:], results[0][1:]):
            assert torch.equal(a, b), name


def test_lazy_and_virtual_batchnorm_plans_match_the_materialised_plan(monkeypatch):
    """Three lowerings of the training forward must agree (a materialised plan run twice is bit-identical; the other two differ
    from it only by the summation order inside their convolution kernels, which a batch-6 BatchNorm network amplifies to a few
    per cent in the gradients):
      materialised : every BN+ReLU output written by fn_bn_relu_train_fwd (FACENET_LAZY_BN_MAXHW=0);
      lazy (option) : on the <= 17x17 maps the single reader of a BN+ReLU output normalises the raw tensor while staging it
                     and writes the activated tensor once (fn_conv_desc.nrm_z) -- 68 fewer launches (readers with more than 1024 K
                     columns, the two big 3x3 layers of the reduction blocks, keep the separate pass);
      virtual      : FACENET_NORM_ON_LOAD=1, the activated tensors are never written (78 fewer launches).
    For the lazy plan every side-written tensor is also checked element by element against relu(raw*scale + shift) with the
    scale / shift fn_bn_finalize published in the same run: each element written exactly once, none skipped."""
    from tests.util import structured_images
    E, N = 128, 6
    params, _, _ = fo.build_params(E, seed=0)
    x = torch.from_numpy(structured_images(N, seed=7))
    results, launches = [], []
    for mode in ("mat", "mat", "lazy", "virtual"):
        monkeypatch.setenv("FACENET_NORM_ON_LOAD", "1" if mode == "virtual" else "0")
        monkeypatch.setenv("FACENET_LAZY_BN_MAXHW", "0" if mode == "mat" else "17")
        net = Network(embedding_size=E, device="cuda:0", train_dtype=torch.float16)
        net.load_keras_params(params)
        tr = Trainer(net, batch=N, loss="triplet", alpha=0.2, lr=0.01)
        tr.set_images(x)
        tr.step_eager()
        torch.cuda.synchronize()
        results.append((tr.loss_value(), tr.emb.clone(), tr.G.clone(), net.P.clone(), net.S_mean.clone(), net.S_var.clone()))
        launches.append(sum(1 for op in tr.plan.fwd if op.name.startswith("bn_relu_fwd")))
        assert bool(tr.plan.virtual) == (mode == "virtual") and bool(tr.plan.lazy) == (mode == "lazy")
        if mode == "lazy":
            assert any(op.name == "bn_finalize" for op in tr.plan.fwd)
            checked = 0
            for name, ranges in tr.plan.lazy.items():
                b = tr.plan.bufs[name]
                for (c0, Cc) in ranges:
                    o = b.bn_off + c0
                    sc, sh = tr.plan.save_scale[o:o + Cc].cpu(), tr.plan.save_shift[o:o + Cc].cpu()
                    want = torch.relu(b.raw[..., c0:c0 + Cc].float().cpu() * sc + sh)
                    got = b.act[..., c0:c0 + Cc].float().cpu()
                    assert torch.allclose(got, want, rtol=2e-3, atol=1e-3), (name, c0, float((got - want).abs().max()))
                    checked += 1
            assert checked == 68
    assert launches[0] - launches[2] == 68 and launches[0] - launches[3] == 78
    assert torch.equal(results[1][1], results[0][1]) and torch.equal(results[1][2], results[0][2])     # reproducible bit for bit
    for which in (2, 3):
        d = (_rel(results[which][1], results[0][1]), _rel(results[which][2], results[0][2]))
        print(f"plan {which} vs materialised (emb, grad):", d)
        assert d[0] <= 5e-3 and d[1] <= 8e-2
        assert torch.allclose(results[which][4], results[0][4], rtol=1e-3, atol=1e-4) and torch.allclose(results[which][5], results[0][5], rtol=1e-3, atol=1e-4)


def test_autotuned_plan_matches_heuristic_plan(monkeypatch, tmp_path):
    """train.autotune_convs times the nine tile variants of every forward / data-gradient convolution and pins the winner in
    the descriptor; results may differ from the heuristic plan only by summation order.  The tile cache replays the choice."""
    from tests.util import structured_images
    E, N = 128, 6
    params, _, _ = fo.build_params(E, seed=0)
    x = torch.from_numpy(structured_images(N, seed=7))
    cache = tmp_path / "tiles.json"
    results, tiles = [], []
    for mode in ("0", "0", "1", "cached"):
        monkeypatch.setenv("FACENET_AUTOTUNE", "0" if mode == "0" else "1")
        if mode != "0":
            monkeypatch.setenv("FACENET_TUNE_CACHE", str(cache))
        net = Network(embedding_size=E, device="cuda:0", train_dtype=torch.float16)
        net.load_keras_params(params)
        tr = Trainer(net, batch=N, loss="triplet", alpha=0.2, lr=0.01)
        tr.set_images(x)
        tr.step_eager()
        torch.cuda.synchronize()
        results.append((tr.emb.clone(), tr.G.clone()))
        tiles.append(dict(tr.tiles))
    # 0 = the library's own choice won (only offered where that is the halo-tile kernel, which competes with the nine tiles)
    assert tiles[0] == {} and len(tiles[2]) > 200 and all(t == 0 or (t // 1000 in (128, 64, 32) and t % 1000 in (128, 64, 32)) for t in tiles[2].values())
    assert all(t != 0 or "conv2d/Conv2d_" in k for k, t in tiles[2].items())            # only stem layers are halo-eligible
    assert tiles[3] == tiles[2] and cache.is_file()                    # second tuned trainer: read back, not re-timed
    assert torch.equal(results[1][0], results[0][0]) and torch.equal(results[1][1], results[0][1])      # same plan: same bits
    assert torch.equal(results[3][0], results[2][0]) and torch.equal(results[3][1], results[2][1])      # cached tiles: the tuned plan again
    d = (_rel(results[2][0], results[0][0]), _rel(results[2][1], results[0][1]))
    # other tiles = another summation order; a batch-6 BatchNorm network amplifies the last-bit differences to a few per cent
    assert d[0] <= 5e-3 and d[1] <= 8e-2, d


GROUPED_STEP_GRAD_BOUND = 1e-2      # measured 3.6e-3 (the Block17 `up` biases); rb_scale off by 5 % in the fusion gives 7e-2


def test_grouped_and_fused_step_matches_the_unfused_step(monkeypatch):
    """The launches Trainer.step issues -- grouped forward / data-gradient convolutions (train.group_convs), merged sibling data
    gradients and the residual backward fused into their epilogue (engine._fuse_residual) -- against the plain lowering
    (FACENET_FUSE_RESIDUAL_BWD=0, FACENET_MERGE_SIBLINGS=0, Trainer(group_wgrad=False)), one f16 step at batch 6.  Grouping
    changes no forward bit and the fusion is backward only, so loss and embeddings are identical; the gradients differ by
    summation order and one rounding of the fused data gradients."""
    E, N = 128, 6
    params, _, _ = fo.build_params(E, seed=0)
    from tests.util import structured_images
    x = torch.from_numpy(structured_images(N, seed=7))
    results = []
    for prod in (True, False):
        monkeypatch.setenv("FACENET_FUSE_RESIDUAL_BWD", "1" if prod else "0")
        monkeypatch.setenv("FACENET_MERGE_SIBLINGS", "1" if prod else "0")
        net = Network(embedding_size=E, device="cuda:0", train_dtype=torch.float16)
        net.load_keras_params(params)
        tr = Trainer(net, batch=N, loss="triplet", alpha=0.2, lr=0.01, group_wgrad=prod)
        tr.set_images(x)
        names = [op.name for op in tr.step_ops]
        # 21 residual blocks; fused: every block whose output feeds merged sibling 1x1 data gradients (the next block's towers,
        # Reduction-B's three 1x1 towers); left: the last Block35 (Reduction-A has one 1x1 tower) and the last Block8 (avg pool)
        assert sum(n.startswith("residual_bwd") for n in names) == (2 if prod else 21)
        grouped = sum(n.startswith(("conv_fwd_grouped", "conv_dgrad_grouped")) for n in names)
        assert (grouped > 0) == prod, grouped
        tr.step_eager()
        torch.cuda.synchronize()
        results.append((tr.loss_value(), tr.emb.clone(), net.export_keras_grads(tr.G)))
    assert results[0][0] == results[1][0] and torch.equal(results[0][1], results[1][1])
    diffs = sorted(((_rel(results[0][2][k], results[1][2][k]), k) for k in results[1][2] if float(results[1][2][k].norm()) > 0), reverse=True)
    worst = diffs[0]
    print("largest per-variable gradient differences (relative L2):", diffs[:5])
    assert worst[0] <= GROUPED_STEP_GRAD_BOUND, worst
