"""Inception-ResNet-v2: host-side checks (no GPU): variable counts, map sizes, the slim name table, v1 plans unchanged; the
restatement's stage entry points and shared selections, planted backward errors against the block-level bound, the tail's
measured bound, and single-stage plans against the whole model's."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from facenet_amd.engine import Network
from facenet_amd.engine_v2 import BlockNetworkV2, NetworkV2, build_network, map_sizes, network_class
from tests import irv2_oracle as ro
from tests.conv_dispatch_signature import conv_ops
from tests.irv2_oracle import param_names
from tests.plan_signature import _canon, _spans, _stub_network, _tensors, signature

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "v1_plan_signature.json")


@pytest.mark.parametrize("E, counts", [(128, (54533728, 54472928)), (512, (55124704, 55063136))])
def test_variable_counts(E, counts):
    assert NetworkV2(E, allocate=False, device="cpu").count_variables() == counts


def test_variable_breakdown_E128():
    net = NetworkV2(128, allocate=False, device="cpu")
    Ls = list(net.layers.values())
    assert sum(L.cout_real * L.kh * L.kw * L.cin_real for L in Ls) == 54396768
    assert sum(L.cout_real for L in Ls if L.has_bias) == 45760
    assert sum(L.cout for L in Ls if L.has_bn) == 30400 == net.CB


def test_map_sizes():
    assert map_sizes(160) == (17, 8, 3)
    assert map_sizes(299) == (35, 17, 8)
    for size, (s5, s6, s7) in ((160, (17, 8, 3)), (299, (35, 17, 8))):
        net = NetworkV2(128, image_size=size, allocate=False, device="cpu")
        assert net.count_variables() == (54533728, 54472928)     # whole-map pool: the head does not depend on the size
    with pytest.raises(ValueError):
        NetworkV2(128, image_size=60, allocate=False, device="cpu")


def test_config_keys_and_momentum():
    net = NetworkV2(allocate=False, device="cpu", config={"repeat": [1, 2, 1], "keep_probability": 0.8, "weight_decay": 1e-3,
                                                          "mixed_5a": {"branch": [[32], [16, 24], [16, 24, 32], [16]]}})
    assert net.E == 512 and net.keep_probability == 0.8 and net.l2_weight == 5e-4
    assert net.layers["Mixed_5a/Branch_1/Conv2d_0b_5x5"].cout == 24
    assert "Repeat_1/block17_2/Conv2d_1x1" in net.layers and "Repeat_1/block17_3/Conv2d_1x1" not in net.layers
    assert net.bn_momentum == 0.995 and Network.bn_momentum == 0.99
    assert net.layers["Repeat/block35_1/Conv2d_1x1"].cout == 104      # up width = the trunk's (Mixed_5a concat)


EXAMPLES = [
    "InceptionResnetV2/Conv2d_1a_3x3/weights",
    "InceptionResnetV2/Conv2d_1a_3x3/BatchNorm/beta",
    "InceptionResnetV2/Conv2d_1a_3x3/BatchNorm/moving_mean",
    "InceptionResnetV2/Conv2d_1a_3x3/BatchNorm/moving_variance",
    "InceptionResnetV2/Mixed_5a/Branch_1/Conv2d_0b_5x5/weights",
    "InceptionResnetV2/Repeat/block35_1/Branch_2/Conv2d_0c_3x3/weights",
    "InceptionResnetV2/Repeat/block35_1/Conv2d_1x1/weights",
    "InceptionResnetV2/Repeat/block35_1/Conv2d_1x1/biases",
    "InceptionResnetV2/Repeat/block35_10/Conv2d_1x1/biases",
    "InceptionResnetV2/Repeat_1/block17_20/Branch_1/Conv2d_0c_7x1/weights",
    "InceptionResnetV2/Repeat_2/block8_9/Branch_1/Conv2d_0b_1x3/weights",
    "InceptionResnetV2/Block8/Branch_0/Conv2d_1x1/weights",
    "InceptionResnetV2/Block8/Conv2d_1x1/biases",
    "InceptionResnetV2/Bottleneck/weights",
    "InceptionResnetV2/Bottleneck/BatchNorm/beta",
]


def test_name_table_is_a_bijection():
    net = NetworkV2(128, nrof_classes=10, allocate=False, device="cpu")
    table = net.variable_table()
    names, keys = [k for k, _ in table], [i for _, i in table]
    assert len(set(names)) == len(names) and len(set(keys)) == len(keys)
    engine = []
    for L in net.layers.values():
        engine.append(L.name + "/kernel")
        if L.has_bias:
            engine.append(L.name + "/bias")
        if L.has_bn:
            engine += [f"{L.name}/bn/{v}" for v in ("beta", "moving_mean", "moving_variance")]
    assert sorted(keys) == sorted(engine)
    for ex in EXAMPLES:
        assert ex in names, ex
    assert "Logits/weights" in names and "Logits/biases" in names
    assert not any(n.startswith("InceptionResnetV2/Repeat/block35_0") for n in names)


def test_restatement_names_match_table():
    net = NetworkV2(128, allocate=False, device="cpu")
    assert param_names(128) == [i for _, i in net.variable_table()]


def test_module_selection():
    assert network_class(None) is Network
    assert network_class("facenet.models.inception_resnet_v1") is Network
    assert network_class("facenet.models.inception_resnet_v2") is NetworkV2
    assert network_class("facenet_amd.models.inception_resnet_v2") is NetworkV2
    with pytest.raises(ValueError):
        network_class("facenet.models.squeezenet")
    from facenet_amd.config import Config
    net = build_network(Config({"module": "facenet.models.inception_resnet_v2", "config": {"repeat": [1, 1, 1]}}), 128,
                        allocate=False, device="cpu")
    assert isinstance(net, NetworkV2) and net.E == 128 and net.cfg["repeat"] == [1, 1, 1]


def test_v2_plan_lowers_on_host():
    """A v2 training plan (with dropout) and an inference plan lower without a GPU; dropout only in training."""
    net = NetworkV2(128, allocate=False, device="cpu", config={"repeat": [1, 1, 1]})
    tr = signature(net, 6, True)
    names = [op[0] for op in tr]
    assert "dropout_fwd" in names and "dropout_bwd" in names
    assert "avgpool3x3s1_fwd" in names and "avgpool3x3s1_bwd" in names
    inf = signature(NetworkV2(128, allocate=False, device="cpu", config={"repeat": [1, 1, 1]}), 6, False)
    assert "dropout_fwd" not in [op[0] for op in inf]
    no_drop = signature(NetworkV2(128, allocate=False, device="cpu", config={"repeat": [1, 1, 1], "keep_probability": 1.0}), 6, True)
    assert not any(op[0].startswith("dropout") for op in no_drop)


def test_v1_launch_lists_unchanged():
    """v1 plans (training + backward, inference layer-wise and with fused blocks) lower to the same launches with the same
    arguments as before the v2 refactor (tests/golden/v1_plan_signature.json, recorded on the previous engine)."""
    with open(GOLDEN) as fh:
        golden = json.load(fh)
    for key, N, tr, E in (("train_triplet_6_E128", 6, True, 128), ("infer_6_E512", 6, False, 512), ("infer_32_E128", 32, False, 128)):
        sig = signature(Network(E, allocate=False, device="cpu"), N, tr)
        assert len(sig) == golden[key]["ops"], key
        assert hashlib.sha256(json.dumps(sig, sort_keys=True).encode()).hexdigest() == golden[key]["sha256"], key


# ---- the block level (tests/test_gpu_irv2_blocks.py) without a GPU: the restatement's stage entry points, its mask plumbing, what
# the bound can see, and that a stage lowered alone is the stage inside the model ------------------------------------------------
def _block_net(case, dt=torch.bfloat16, N=None):
    stages, HW, Cc, _, keep = ro.BLOCK_CASES[case]
    return BlockNetworkV2(stages, HW, HW, Cc, embedding_size=ro.BLOCK_E, config={"keep_probability": keep}, allocate=False, device="cpu",
                          seed=ro.BLOCK_SEED, train_dtype=dt)


def test_stage_entry_points_equal_the_whole_forward():
    """stem() and then stage() call by call reproduce forward()'s end points and embedding bit for bit (repeat [1,1,1], fp32)."""
    cfg = dict(ro.CFG, repeat=[1, 1, 1])
    params = NetworkV2(128, allocate=False, device="cpu", config={"repeat": [1, 1, 1]}).init_keras_params(3)
    x = torch.from_numpy(np.random.default_rng(0).standard_normal((2, 160, 160, 3)).astype(np.float32))
    for training in (False, True):
        ep = {}
        emb = ro.IRv2(params, cfg=cfg).forward(x, training=training, preprocessed=True, end_points=ep)
        o = ro.IRv2(params, cfg=cfg)
        y = o.stem(x, training, preprocessed=True)
        got = {}
        for stage in ["mixed_5a", "block35", "mixed_6a", "block17", "mixed_7a", "block8", "block8_last", "conv_7b", "head"]:
            y = o.stage(y, stage, training)
            got[stage] = y
        for stage, name in (("mixed_5a", "Mixed_5a"), ("mixed_6a", "Mixed_6a"), ("mixed_7a", "Mixed_7a"), ("conv_7b", "Conv2d_7b_1x1")):
            assert torch.equal(got[stage], ep[name]), name
        assert ep["Mixed_5a"].shape == (2, 320, 17, 17) and ep["Mixed_7a"].shape == (2, 2080, 3, 3)
        assert torch.equal(y, emb) and emb.shape == (2, 128) and float(emb.abs().max()) > 0


def test_shared_selections_are_an_identity_on_the_own_ones():
    """The restatement's own ReLU sets as ``relu_masks`` and its own trunks as the max-pool selection sources give the output and
    the gradients of passing none (a max-pool gradient adds up to four windows per pixel, in another order: 1e-6)."""
    case, dt = "chain_17_7a_8", torch.bfloat16
    params, tr, x, dout, drop = ro.block_operands(_block_net(case, dt), case, dt)
    y0, dx0, g0, o = ro.block_reference(params, tr, case, x, dout, dt, drop)
    assert {"Mixed_7a"} == set(o.own_pool) and "Repeat_1/block17_1" in o.own_relu and "Mixed_7a/Branch_2/Conv2d_1a_3x3" in o.own_relu
    assert "Repeat_2/block8_1/Conv2d_1x1" not in o.own_relu
    y1, dx1, g1, _ = ro.block_reference(params, tr, case, x, dout, dt, drop, relu_masks=o.own_relu, pool_src=o.own_pool)
    assert torch.equal(y0, y1)
    assert ro.rel(dx1, dx0) < 1e-6 and set(g0) == set(g1)
    for k in g0:
        assert ro.rel(g1[k], g0[k]) < 1e-6, k
    # ... and the selection really is taken from the source: another trunk selects other pixels
    other = {"Mixed_7a": torch.flip(o.own_pool["Mixed_7a"], dims=(2, 3))}
    _, dx2, _, _ = ro.block_reference(params, tr, case, x, dout, dt, drop, relu_masks=o.own_relu, pool_src=other)
    assert ro.rel(dx2, dx0) > 0.1


def test_maxpool_selection_takes_the_first_maximum():
    """_MaxPoolSelected on a map of ties: the first maximum in scan order (ky, kx) gets the whole gradient of its window, as
    fn_maxpool3x3s2_bwd gives it (and as torch's CPU max-pool does)."""
    x = torch.zeros(1, 1, 5, 5)
    x[0, 0, 1, 2] = x[0, 0, 2, 1] = 1.0                      # window (0, 0) sees both: (ky, kx) = (1, 2) comes before (2, 1)
    xr = x.clone().requires_grad_(True)
    y = ro._MaxPoolSelected.apply(xr, x)
    g = torch.tensor([[[[1.0, 2.0], [4.0, 8.0]]]])
    y.backward(g)
    ref = x.clone().requires_grad_(True)
    torch.nn.functional.max_pool2d(ref, 3, 2).backward(g)
    assert torch.equal(y.detach(), torch.nn.functional.max_pool2d(x, 3, 2))
    assert torch.equal(xr.grad, ref.grad)
    assert xr.grad[0, 0, 1, 2] == 1.0 + 2.0 and xr.grad[0, 0, 2, 1] == 4.0 and xr.grad[0, 0, 2, 2] == 8.0     # all-zero window: its first pixel


class _AvgPoolIncludePadBackward(torch.autograd.Function):
    """AvgPool 3x3 / 1 / SAME dividing by the in-map taps forward, by 9 everywhere backward (the planted error)."""

    @staticmethod
    def forward(ctx, x):
        return torch.nn.functional.avg_pool2d(x, 3, 1, 1, count_include_pad=False)

    @staticmethod
    def backward(ctx, g):
        return torch.nn.functional.avg_pool2d(g, 3, 1, 1, count_include_pad=True)       # the uniform 1/9 stencil is its own adjoint


class _RoundGradient(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, dt):
        ctx.dt = dt
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return g.to(ctx.dt).float(), None


class _ResidualScaleOnTrunk(torch.autograd.Function):
    """x + scale * up whose backward scales the trunk's gradient instead of up's (the planted error)."""

    @staticmethod
    def forward(ctx, x, up, scale):
        ctx.scale = scale
        return x + scale * up

    @staticmethod
    def backward(ctx, g):
        return ctx.scale * g, g, None


def _planted(kind):
    """The restatement with one error of the backward pass planted (the forward is the reference's)."""
    class Planted(ro.IRv2):
        def _avgpool3(self, x):
            if kind == "avgpool_tower_dropped":
                x = x.detach()
            if kind == "avgpool_include_pad":
                return ro._q(_AvgPoolIncludePadBackward.apply(x), self.dt)
            return super()._avgpool3(x)

        def _maxpool(self, x, pre=None):
            if kind == "maxpool_dropped":
                x = x.detach()
            if kind == "rounded_after_each_producer":
                x = _RoundGradient.apply(x, self.dt)
            return super()._maxpool(x, pre)

        def _tower(self, x, pre, i, tower, training):
            if pre.startswith("Mixed"):
                if kind == "one_tower_1x1_missing" and i == 1:
                    x = x.detach()
                if kind == "rounded_after_each_producer":
                    x = _RoundGradient.apply(x, self.dt)
            return super()._tower(x, pre, i, tower, training)

        def _residual(self, x, up, pre, scale, relu):
            if kind == "residual_scale_on_dtrunk":
                y = _ResidualScaleOnTrunk.apply(x, up, scale)
                return ro._q(self._relu(y, pre) if relu else y, self.dt)
            return super()._residual(x, up, pre, scale, relu)
    return Planted


# (case, planted error, whether tol_g sees it).  Rounding the trunk gradient after each of its producers instead of where the
# device rounds moves it by a fraction of a storage ulp (2^-9 bf16 / 2^-12 f16 relative, against tol_g = 1e-2 / 2e-3): the block
# test cannot see it; the element-wise accumulate cases of tests/test_gpu_conv.py hold that rounding.
PLANTED = [
    ("mixed_5a", "avgpool_tower_dropped", True), ("mixed_5a", "avgpool_include_pad", True), ("mixed_5a", "one_tower_1x1_missing", True),
    ("mixed_5a", "rounded_after_each_producer", False),
    ("chain_17_7a_8", "maxpool_dropped", True), ("chain_17_7a_8", "one_tower_1x1_missing", True), ("chain_17_7a_8", "residual_scale_on_dtrunk", True),
    ("chain_17_7a_8", "rounded_after_each_producer", False),
    ("block8", "residual_scale_on_dtrunk", True),
]
_REFERENCES = {}


def _reference_of(case, dt):
    if (case, dt) not in _REFERENCES:
        ops = ro.block_operands(_block_net(case, dt), case, dt)
        _REFERENCES[(case, dt)] = (ops, ro.block_reference(ops[0], ops[1], case, *ops[2:4], dt, ops[4]))
    return _REFERENCES[(case, dt)]


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("case,kind,visible", PLANTED, ids=[f"{c}-{k}" for c, k, _ in PLANTED])
def test_planted_backward_errors_against_the_block_bound(case, kind, visible, dt):
    """Each planted error moves dX or a dW of the reference by more than tol_g, the bound of the GPU comparison on shared sets --
    except the one listed as invisible, which must stay inside it (if that changes, PLANTED and DESIGN.md change with it)."""
    (params, tr, x, dout, drop), (y, dx, g, o) = _reference_of(case, dt)
    yp, dxp, gp, _ = ro.block_reference(params, tr, case, x, dout, dt, drop, cls=_planted(kind))
    assert torch.equal(yp, y)                                 # only the backward pass is wrong
    errs = {k: ro.rel(gp[k], g[k]) for k in g if g[k].norm() > 1e-6}
    errs["dX"] = ro.rel(dxp, dx)
    worst = max(errs, key=errs.get)
    tol = ro.tol_g(case, dt)
    print(f"{case} {kind} {dt}: dX {errs['dX']:.2e}, worst {worst} {errs[worst]:.2e}, tol_g {tol:.1e}: margin x{errs[worst] / tol:.2f}")
    if visible:
        assert errs[worst] > tol, f"{kind} on {case} stays inside tol_g: the block test cannot see it"
    else:
        assert 0 < errs[worst] < tol, f"{kind} on {case} is now outside tol_g: list it as visible"


@pytest.mark.parametrize("case", sorted(ro.TAIL_MEASURED, key=str), ids=lambda c: f"{c[0]}-{str(c[1]).split('.')[-1]}")
def test_tail_bounds_follow_their_measurements(case):
    """irv2_oracle.TAIL_MEASURED holds what ulp_perturbed_distance measures (within 10 %: CPU summation order) and the tail's
    gradient bound is twice that.  The forward bound is tol_y of the other cases, except where the fp64 evaluation of the same
    rounded model lies further than tol_y from the fp32 one: that is the bf16 tail without dropout alone, FP64_FORWARD holds the
    measured distance, and the bound is four times it."""
    name, dt = case
    net = _block_net(name, dt)
    e_y, e_g = ro.ulp_perturbed_distance(net, name, dt)
    d64 = ro.fp64_forward_distance(net, name, dt)
    print(f"{name} {dt}: one-ulp perturbation moves the worst gradient by {e_g:.3e} (the output by {e_y:.3e}); "
          f"fp64 evaluation of the rounded model: forward {d64:.3e} from the fp32 one")
    m_g = ro.TAIL_MEASURED[case]
    assert abs(e_g - m_g) < 0.1 * m_g and ro.tol_g(name, dt) == 2 * m_g > ro.TOL[dt][1]
    if case in ro.FP64_FORWARD:
        assert d64 > ro.TOL[dt][0] and abs(d64 - ro.FP64_FORWARD[case]) < 0.1 * d64 and ro.tol_y(name, dt) == 4 * ro.FP64_FORWARD[case]
    else:
        assert ro.tol_y(name, dt) == ro.TOL[dt][0]


def test_only_the_measured_cases_leave_the_block_bounds():
    assert set(ro.FP64_FORWARD) == {("tail_keep_1", torch.bfloat16)}
    for case in ro.BLOCK_CASES:
        for dt in (torch.float16, torch.bfloat16):
            if (case, dt) not in ro.FP64_FORWARD:
                assert ro.tol_y(case, dt) == ro.TOL[dt][0]
            if (case, dt) not in ro.TAIL_MEASURED:
                assert ro.tol_g(case, dt) == ro.TOL[dt][1]


# ---- a stage alone is the stage inside the model ----
_SIZE_FIELDS = ("stats_sq_off", "stats_rep_stride", "bn_sq_off", "bn_rep_stride")      # strides of the BN channel space: its size differs
_MODELS = {}


def _lowered(net, N):
    _stub_network(net)
    plan = net.plan(N, training=True)
    plan.build_backward(torch.zeros(N, net.E))
    return plan


def _descriptors(net, plan, rename):
    """{launch name: {field: value}} of the convolution launches: numbers as they are, pointers as (tensor role, byte offset)
    for activations / gradients / scratch (``rename``: buffer name -> name) and as the role alone for the parameter-sized tensors."""
    spans = _spans(_tensors(net, plan))
    out = {}
    for op in conv_ops(plan.fwd + plan.bwd):
        row = {}
        for f, v in _canon(op.keep[0], spans):
            if f in _SIZE_FIELDS:
                continue
            if isinstance(v, tuple) and v[0] == "ptr":
                role = v[1].split(".")
                if role[0] == "buf":
                    v = ("buf", rename.get(".".join(role[1:-1]), ".".join(role[1:-1])), role[-1], v[2])
                elif role[0] in ("net", "plan"):
                    v = (v[1],)
            row[f] = v
        assert op.name not in out
        out[op.name] = row
    return out


@pytest.mark.parametrize("case", sorted(ro.BLOCK_CASES))
def test_a_stage_alone_is_the_stage_inside_the_model(case):
    """Every convolution launch of a single-stage plan (forward, data gradient, weight gradient) has, field by field, the
    descriptor of the launch of the same name inside NetworkV2(...).plan(N, training=True): geometry, row strides, channel
    offsets, kind, residual and sibling fields; and a block inside a chain keeps its residual backward fused or unfused as the
    model has it at that boundary.  One difference is the plan's outer edge: where the model's stage input is itself a block
    output, the model fuses that block's residual backward into the stage's first data gradient (rb_*), the lone stage has no
    such block (a lone Block8 and a lone Mixed_7a)."""
    stages, HW, Cc, N, keep = ro.BLOCK_CASES[case]
    repeat = [2, 2, 2] if case.endswith("_x2") else [1, 1, 1]
    size = 160 if HW in (17, 8, 3) and not case.startswith("g299") else 299
    key = (size, N, repeat[0], keep)
    if key not in _MODELS:
        net = NetworkV2(ro.BLOCK_E, allocate=False, device="cpu", image_size=size, config={"repeat": repeat, "keep_probability": keep})
        _MODELS[key] = (net, _lowered(net, N))
    model, mplan = _MODELS[key]
    alone = _block_net(case)
    aplan = _lowered(alone, N)
    first = next(r for r in aplan.recs if r.x is not None and r.x.buf.name == "trunk")
    minput = next(r.x.buf for r in mplan.recs if r.layer is not None and first.layer is not None and r.layer.name == first.layer.name) \
        if first.layer is not None else next(r.x.buf for r in mplan.recs if r.kind == first.kind and r.y.buf.name == first.y.buf.name)
    assert (minput.H, minput.W, minput.C) == (HW, HW, Cc)
    a, m = _descriptors(alone, aplan, {"trunk": "INPUT"}), _descriptors(model, mplan, {minput.name: "INPUT"})
    assert set(a) <= set(m) and len(a) >= 3 * len([L for L in alone.layers.values()]) - len(stages) - 3, sorted(set(a) - set(m))
    edge = 0
    for name, row in a.items():
        want = dict(m[name])
        if want["rb_prev"] and want["rb_prev"][:2] == ("buf", "INPUT"):        # the outer edge (see above)
            edge += 1
            assert not row["rb_prev"] and row["accumulate"] == 1 and want["accumulate"] == 0
            for f in want:
                if f.startswith("rb_") or f == "accumulate":
                    want[f] = row[f]
        diff = {f: (row[f], want[f]) for f in row if row[f] != want[f]}
        assert not diff, (name, diff)
    # Block8 follows block8_<r> and Mixed_7a follows block17_<r>: both complete the block output's gradient with a sibling group
    # (Mixed_6a has no such group: the Block35's residual backward is a launch of its own there, nothing of it in a descriptor)
    assert edge == (1 if stages[0] in ("block8_last", "mixed_7a") else 0)
    # residual backward launches of the blocks inside the chain (every block but the last of the plan): as in the model
    blocks = [r.layer.name for r in aplan.recs if r.kind == "conv" and r.extra.get("kind") == "resid"]
    unfused = lambda plan: {op.name for op in plan.bwd if op.name.startswith("residual_bwd:")}
    for b in blocks[:-1]:
        assert (("residual_bwd:" + b) in unfused(aplan)) == (("residual_bwd:" + b) in unfused(mplan)), b
