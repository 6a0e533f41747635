"""Inception-ResNet-v2 at the block level: every stage alone, two chains across a reduction and the tail, forward and backward,
f16 and bf16, against fp32 autograd on identically rounded operands (tests/irv2_oracle.py: IRv2.stages).

Each case is lowered ALONE by engine_v2.BlockNetworkV2 -- the calls NetworkV2._topology makes, so the production lowering, kernel
choice and fusions run -- on the 160-pixel maps (17 / 8 / 3) and on the 299-pixel ones (35 / 17 / 8).  As in
tests/test_gpu_blocks.py the comparison runs twice: on the restatement's own ReLU sets (the forward must agree; the gradient is
then bounded by the sign flips, 10 sqrt(e_y) + tol_g) and on the device's sets (ReLU active sets, and inside a chain the window
selection of the max-pool, taken from the device's stored activations), where the backward arithmetic is held to tol_g.

Bounds (relative L2): output 1e-3 (f16) / 4e-3 (bf16); dX and every dW / dbeta / dbias 2e-3 / 1e-2 -- the numbers of
tests/test_gpu_blocks.py for the same kernels and storage types.  The tails end in the Bottleneck BatchNorm over N = 48 samples;
their gradient bound is twice the distance the reference itself moves under a one-ulp change of its input, measured on the CPU
without the device (irv2_oracle.TAIL_MEASURED: 1.8e-3 f16 / 1.4e-2 .. 1.5e-2 bf16, so 3.6e-3 / 2.9e-2).  Their forward bound is the
one above, with one measured exception: for the bf16 tail without dropout the fp64 evaluation of the same rounded model lies
7.05e-3 from the fp32 evaluation (irv2_oracle.FP64_FORWARD), so two correct evaluations are further apart than 4e-3; that case is
held to four times the measured distance, 2.8e-2 (measured on the device: 6.7e-3).
PARITY UNPINNED by the reference (no vectors for v2).

Measured on MI355X: DESIGN.md section 4, "v2 block level"."""
import ctypes as C

import numpy as np
import pytest
import torch

from facenet_amd import _lib
from facenet_amd.engine_v2 import BlockNetworkV2
from tests import irv2_oracle as ro
from tests.conv_dispatch_signature import conv_ops

pytestmark = pytest.mark.gpu

OPS = {"conv_fwd": 0, "conv_dgrad": 1}


def _nchw(t):
    return t.float().cpu().permute(0, 3, 1, 2).contiguous()


def _device_sets(plan):
    """(ReLU active sets, max-pool selection sources) of the device, keyed as the restatement keys them."""
    masks, pool_src = {}, {}
    for r in plan.recs:
        if r.kind == "conv" and r.extra.get("kind") == "bn" and any(b[2] for b in plan.bn_ranges.get(r.y.buf.name, [])):
            masks[r.layer.name] = _nchw(r.y.buf.act[..., r.y.c0:r.y.c0 + r.y.C] > 0)
        elif r.kind == "conv" and r.extra.get("kind") == "resid" and r.extra["relu"]:
            masks[r.layer.name[:-len("/Conv2d_1x1")]] = _nchw(r.y.buf.act > 0)
        elif r.kind == "maxpool":
            pool_src[r.y.buf.name[:-len("/out")]] = _nchw(r.x.buf.act[..., r.x.c0:r.x.c0 + r.x.C])
    return masks, pool_src


def _kernel_choice(lib, plan):
    """{launch name: fn_conv2d_variant} of every convolution's forward and data-gradient descriptor."""
    out = {}
    for op in conv_ops(plan.fwd + plan.bwd):
        kind = op.name.split(":")[0]
        if kind in OPS:
            out[op.name] = lib.fn_conv2d_variant(C.byref(op.keep[0]), OPS[kind])
    return out


def _check_launches(case, plan, choice):
    bwd = [op.name for op in plan.bwd]
    if case == "g299_block35":          # <= 64 source channels on a 35x35 map: the halo-tile kernel
        k3 = [n for n in choice if n.startswith("conv_fwd:") and n.endswith("_3x3")]
        assert len(k3) == 3 and all(_lib.variant_is_halo(choice[n]) for n in k3), {n: choice[n] for n in k3}
    if case == "chain_17_7a_8":         # the Block17's residual backward runs in the epilogue of Mixed_7a's three-source data gradient
        assert "residual_bwd:Repeat_1/block17_1/Conv2d_1x1" not in bwd
        m7 = [op for op in plan.bwd if op.name.startswith("conv_dgrad:") and "Mixed_7a" in op.name and op.keep[0].dy2 and op.keep[0].dy3]
        assert len(m7) == 1 and m7[0].keep[0].rb_prev and bwd.index("maxpool_bwd") < bwd.index(m7[0].name)
    if case == "chain_35_6a_17":        # no sibling group completes the Block35 output's gradient: a launch of its own
        assert "residual_bwd:Repeat/block35_1/Conv2d_1x1" in bwd
    if case == "mixed_5a":              # four producers of the trunk gradient
        assert "avgpool3x3s1_bwd" in bwd and sum(bool(op.name.startswith("conv_dgrad:") and op.keep[0].dy3) for op in plan.bwd) == 1


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("case", list(ro.BLOCK_CASES))
def test_v2_stage_forward_backward_against_rounded_autograd(lib, case, dt):
    stages, HW, Cc, N, keep = ro.BLOCK_CASES[case]
    net = BlockNetworkV2(stages, HW, HW, Cc, embedding_size=ro.BLOCK_E, config={"keep_probability": keep}, device="cuda:0",
                         train_dtype=dt, seed=ro.BLOCK_SEED)
    assert net.bn_momentum == 0.995
    params, trainable, x, dout, drop = ro.block_operands(net, case, dt)
    net.load_keras_params(params)
    plan = net.plan(N, training=True)
    net.alloc_grads()
    trunk, out = plan.bufs["trunk"], plan.embedding.buf
    head = stages[-1] == "head"
    trunk.act.copy_(x)
    st = net.stream()
    plan.ws.zero_(); plan.ws_b.zero_()
    plan.run_ops(plan.fwd, st)
    demb = dout.cuda() if head else None
    if not head:
        out.grad.copy_(dout)
    plan.build_backward(demb)
    plan.run_ops(plan.bwd, st)
    torch.cuda.synchronize()

    choice = _kernel_choice(lib, plan)
    print(f"{case} {dt} kernels: " + ", ".join(f"{n} {v}" for n, v in choice.items()))
    _check_launches(case, plan, choice)

    masks, pool_src = _device_sets(plan)
    mine = net.export_keras_grads(net.G)
    y_dev = out.act.float().cpu().view(N, -1) if head else out.act.float().cpu()
    tol_y, tol_g = ro.tol_y(case, dt), ro.tol_g(case, dt)
    for shared in (False, True):
        y_ref, dx_ref, grads, orc = ro.block_reference(params, trainable, case, x, dout, dt, drop, masks if shared else None,
                                                       pool_src if shared else None)
        if shared:        # every device set reached the restatement under its key: none fell back to the restatement's own selection
            assert set(pool_src) == set(orc.own_pool) and set(masks) == set(orc.own_relu), (set(masks) ^ set(orc.own_relu), set(pool_src) ^ set(orc.own_pool))
            assert all(masks[k].shape == orc.own_relu[k].shape for k in masks) and all(pool_src[k].shape == orc.own_pool[k].shape for k in pool_src)
        e_y = ro.rel(y_dev, y_ref)
        e_dx = ro.rel(trunk.grad.float().cpu(), dx_ref)
        errs = {k: ro.rel(mine[k], g) for k, g in grads.items() if g.norm() > 1e-6 and not (head and k == ro.ZERO_BIAS)}
        worst = max(errs, key=errs.get)
        print(f"{case} N={N} {dt} {'device sets' if shared else 'own sets   '}: out {e_y:.2e}  dX {e_dx:.2e}  "
              f"worst dW {worst} {errs[worst]:.2e}  median {np.median(list(errs.values())):.2e}  (bound {tol_y:.1e} / {tol_g:.2e})")
        assert e_y < tol_y
        assert len(errs) >= len(net.layers)          # every kernel has a gradient
        bound = tol_g if shared else 10 * np.sqrt(e_y) + tol_g
        assert e_dx < bound
        for k, e in errs.items():
            assert e < bound, (k, e, shared)
        if head:      # zero in exact arithmetic (irv2_oracle.ZERO_BIAS): held against the terms it sums, not against its own residue
            scale = float(orc.dup_abs["Block8"].norm())
            e0 = float((mine[ro.ZERO_BIAS] - grads[ro.ZERO_BIAS]).norm()) / scale
            print(f"  {ro.ZERO_BIAS}: |device - reference| / |sum of |terms|| {e0:.2e}")
            assert e0 < bound
    # moving statistics: momentum 0.995, biased batch variance, from the un-rounded accumulators.  The batch statistic enters
    # with weight 0.005 and, inside a chain, is taken over activations that differ by at most tol_y = 4e-3 of their O(1)
    # magnitude: 0.005 x 4e-3 = 2e-5 absolute (+ 1e-4 relative).  Momentum 0.99 would move every statistic twice as far.
    new = net.export_keras_params()
    assert len(orc.new_stats) == 2 * sum(L.has_bn for L in net.layers.values())
    dev = max(float((new[k] - v).abs().max()) for k, v in orc.new_stats.items())
    print(f"  moving statistics: max |device - reference| {dev:.2e}")
    for k, v in orc.new_stats.items():
        assert torch.allclose(new[k], v, rtol=1e-4, atol=2e-5), k
