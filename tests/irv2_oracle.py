"""fp32 PyTorch restatement of Inception-ResNet-v2 (test helper), written from the topology table of
facenet/models/inception_resnet_v2.py:40-256 and its yaml, independent of the engine's lowering.

Parameters are a dict of Keras-layout tensors under the engine's keys (``<layer>/kernel`` HWIO, ``<layer>/bias``,
``<layer>/bn/{beta,moving_mean,moving_variance}``; ``Bottleneck/kernel`` is [in, out]).  ``dt`` set: activations and weights
are rounded to that storage type where the HIP path stores them (straight-through), isolating logic from rounding noise.
``dropout_mask`` is the NumPy restatement of the device dropout hash."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import facenet_oracle as fo

BN_EPS, BN_MOMENTUM = 1e-3, 0.995
CFG = {"mixed_5a": [[96], [48, 64], [64, 96, 96], [64]], "mixed_6a": [[384], [256, 256, 384]],
       "mixed_7a": [[256, 384], [256, 288], [256, 288, 320]], "repeat": [10, 20, 9]}


def _mix(h, v):
    h = (h ^ v) & 0xFFFFFFFF
    h ^= h >> 16
    h = (h * 0x7FEB352D) & 0xFFFFFFFF
    h ^= h >> 15
    h = (h * 0x846CA68B) & 0xFFFFFFFF
    h ^= h >> 16
    return h


def dropout_mask(seed, rank, t, N, C, keep):
    """bool [N, C]: lowbias32 fold of (seed, rank, t, n, c) from 0x9E3779B9, kept when below round(keep * 2^32)."""
    n = np.arange(N, dtype=np.uint64)[:, None]
    c = np.arange(C, dtype=np.uint64)[None, :]
    h = np.uint64(0x9E3779B9)
    mix = lambda h, v: _mix(np.asarray(h, dtype=np.uint64), np.asarray(v, dtype=np.uint64) & np.uint64(0xFFFFFFFF))
    h = mix(mix(mix(h, seed), rank), t)
    h = mix(mix(np.broadcast_to(h, (N, 1)), n), c)
    return h < np.uint64(min(int(round(keep * 2.0 ** 32)), 0xFFFFFFFF))


def _q(x, dt):
    return x if dt is None else x + (x.to(dt).to(x.dtype) - x).detach()


def param_names(E=128, nrof_classes=None, cfg=CFG):
    """Engine keys of every variable the restatement reads, in declaration order."""
    return list(IRv2(None, cfg=cfg).declare(E, nrof_classes))


class _MaxPoolSelected(torch.autograd.Function):
    """MaxPool 3x3 / stride 2 / VALID whose window selection is GIVEN: ``src`` (the device's stored trunk activation, NCHW)
    chooses, per window and channel, the FIRST maximum in scan order (ky, kx) -- the tie rule of fn_maxpool3x3s2_fwd / _bwd --
    and x is read, and its gradient written, at that position.  Inside a chain the trunk differs by rounding between the two
    sides, so a window with two near-equal values may select differently; like a ReLU sign flip (quant_oracle._ReluWithMask)
    that moves the whole gradient of the window and is a property of max-pooling, not an error of either side."""

    @staticmethod
    def forward(ctx, x, src):
        N, C, H, W = x.shape
        win = F.unfold(src, 3, stride=2).view(N, C, 9, -1)
        eq = win == win.amax(2, keepdim=True)
        first = (eq & (eq.cumsum(2) == 1)).to(x.dtype)
        ctx.save_for_backward(first)
        ctx.shape = (H, W)
        OH, OW = (H - 3) // 2 + 1, (W - 3) // 2 + 1
        return (F.unfold(x, 3, stride=2).view(N, C, 9, -1) * first).sum(2).view(N, C, OH, OW)

    @staticmethod
    def backward(ctx, g):
        (first,) = ctx.saved_tensors
        N, C = g.shape[:2]
        cols = (first * g.reshape(N, C, 1, -1)).view(N, C * 9, -1)
        return F.fold(cols, ctx.shape, 3, stride=2), None


# stage names of facenet_amd.engine_v2.V2_STAGES -> (scope of block k counted from 1, kind, scale of `up`) of the repeated stages
REPEATED = {"block35": ("Repeat/block35_{}", 0.17), "block17": ("Repeat_1/block17_{}", 0.10), "block8": ("Repeat_2/block8_{}", 0.20)}
TAIL = ("block8_last", "conv_7b", "head")


class IRv2:
    """``masks``: the dropout keep mask [N, 1536].  ``relu_masks``: ReLU active sets to use instead of the restatement's own
    ({0,1} float NCHW, keyed by layer name for a BN+ReLU output and by block prefix for a block output: tests/test_gpu_blocks.py);
    ``pool_src``: reduction prefix ("Mixed_6a" / "Mixed_7a") -> NCHW trunk whose windows select for that stage's max-pool."""

    def __init__(self, params, cfg=CFG, dt=None, keep=1.0, masks=None, relu_masks=None, pool_src=None):
        self.p, self.cfg, self.dt, self.keep, self.masks = params, cfg, dt, keep, masks
        self.relu_masks, self.pool_src = relu_masks or {}, pool_src or {}
        self.own_relu, self.own_pool = {}, {}       # what this evaluation itself selected, under the same keys
        self.dup_abs = {}                           # block prefix -> per-channel sum |d up| (the terms of the bias gradient)
        self.new_stats = {}
        self._names = None

    # ---- declaration (names only) ----
    def declare(self, E, nrof_classes=None):
        self._names = {}
        self.E = E
        self.forward(torch.zeros(1, 160, 160, 3), training=False, preprocessed=True)
        if nrof_classes is not None:
            self._names["classifier/logits/kernel"] = None
            self._names["classifier/logits/bias"] = None
        out, self._names = self._names, None
        return out

    def _get(self, k, shape_fn=None):
        if self._names is not None:
            self._names[k] = None
            return None
        return self.p[k]

    def _relu(self, x, key):
        m = self.relu_masks.get(key)
        self.own_relu[key] = (x.detach() > 0).to(x.dtype)
        if m is None:
            return F.relu(x)
        from tests.quant_oracle import _ReluWithMask
        return _ReluWithMask.apply(x, m)

    def _conv(self, x, name, k, stride=1, padding="same", bias=False, cout=None):
        w = self._get(name + "/kernel")
        b = self._get(name + "/bias") if bias else None
        if self._names is not None:                # declaration walk: shapes only
            kh, kw = k
            oh = x.shape[2] if padding == "same" else (x.shape[2] - kh) // stride + 1
            ow = x.shape[3] if padding == "same" else (x.shape[3] - kw) // stride + 1
            return torch.zeros(x.shape[0], cout, oh, ow)
        w = _q(w, self.dt).permute(3, 2, 0, 1)
        pad = (w.shape[2] // 2, w.shape[3] // 2) if padding == "same" else (0, 0)
        return F.conv2d(x, w, b, stride=stride, padding=pad)

    def _bn(self, y, name, training, relu=True, stored=True):
        """``stored=False``: the convolution output and the normalised output stay fp32 (the Bottleneck: the HIP path keeps the
        Dense output and the embedding in fp32 buffers)."""
        dt = self.dt if stored else None
        beta = self._get(name + "/bn/beta")
        mm, mv = self._get(name + "/bn/moving_mean"), self._get(name + "/bn/moving_variance")
        if self._names is not None:
            return y
        if training:
            mean, var = y.mean(dim=(0, 2, 3)), y.var(dim=(0, 2, 3), unbiased=False)
            self.new_stats[name + "/bn/moving_mean"] = mm * BN_MOMENTUM + mean.detach() * (1 - BN_MOMENTUM)
            self.new_stats[name + "/bn/moving_variance"] = mv * BN_MOMENTUM + var.detach() * (1 - BN_MOMENTUM)
        else:
            mean, var = mm, mv
        z = (_q(y, dt) - mean.view(1, -1, 1, 1)) * torch.rsqrt(var.view(1, -1, 1, 1) + BN_EPS) + beta.view(1, -1, 1, 1)
        return _q(self._relu(z, name) if relu else z, dt)

    def _cbr(self, x, name, cout, k, training, stride=1, padding="same"):
        return self._bn(self._conv(x, name, k, stride, padding, cout=cout), name, training)

    def _maxpool(self, x, pre=None):
        src = self.pool_src.get(pre)
        if pre is not None:
            self.own_pool[pre] = x.detach()
        return F.max_pool2d(x, 3, 2) if src is None else _MaxPoolSelected.apply(x, src)

    def _avgpool3(self, x):
        return _q(F.avg_pool2d(x, 3, 1, 1, count_include_pad=False), self.dt)

    def _tower(self, x, pre, i, tower, training):
        y = x
        for spec in tower:
            if spec[0].startswith("AvgPool"):
                y = self._avgpool3(y)
                continue
            nm, cout, k = spec[:3]
            stride, padding = (spec[3], spec[4]) if len(spec) > 3 else (1, "same")
            y = self._cbr(y, f"{pre}/Branch_{i}/{nm}", cout, k, training, stride, padding)
        return y

    def _towers(self, x, pre, towers, training):
        return [self._tower(x, pre, i, t, training) for i, t in enumerate(towers)]

    def _block(self, x, pre, kind, scale, relu, training):
        from facenet_amd.engine_v2 import V2_BLOCKS
        mixed = torch.cat(self._towers(x, pre, V2_BLOCKS[kind], training), 1)
        up = self._conv(mixed, pre + "/Conv2d_1x1", (1, 1), bias=True, cout=x.shape[1])
        if up.requires_grad:
            up.register_hook(lambda g, pre=pre: self.dup_abs.__setitem__(pre, g.abs().sum(dim=(0, 2, 3))))
        return self._residual(x, up, pre, scale, relu)

    def _residual(self, x, up, pre, scale, relu):
        y = x + scale * up
        return _q(self._relu(y, pre) if relu else y, self.dt)

    def _head(self, x, training):
        x = _q(x.mean(dim=(2, 3)), self.dt)                       # AvgPool_1a over the whole map + flatten
        if training and self.keep < 1.0:
            x = _q(x * torch.as_tensor(self.masks, dtype=x.dtype) / self.keep, self.dt)
        self.pre_logits = x
        w = self._get("Bottleneck/kernel")
        if self._names is not None:
            y = torch.zeros(x.shape[0], self.E, 1, 1)
        else:
            y = (x @ _q(w, self.dt)).view(x.shape[0], -1, 1, 1)
        return self._bn(y, "Bottleneck", training, relu=False, stored=False).view(x.shape[0], -1)

    # ---- stage by stage: what forward() runs below the stem, and what a lone stage or chain runs on an NCHW feature map ----
    def stage(self, x, stage, training, k=1):
        """One stage (a name of engine_v2.V2_STAGES; ``k``: which block of a repeated stage, from 1) on the NCHW map x."""
        from facenet_amd import engine_v2 as v2
        cfg = self.cfg
        if stage == "mixed_5a":
            return torch.cat(self._towers(x, "Mixed_5a", v2.mixed_5a_towers(cfg["mixed_5a"]), training), 1)
        if stage == "mixed_6a":
            return torch.cat(self._towers(x, "Mixed_6a", v2.mixed_6a_towers(cfg["mixed_6a"]), training) + [self._maxpool(x, "Mixed_6a")], 1)
        if stage == "mixed_7a":
            return torch.cat(self._towers(x, "Mixed_7a", v2.mixed_7a_towers(cfg["mixed_7a"]), training) + [self._maxpool(x, "Mixed_7a")], 1)
        if stage in REPEATED:
            scope, scale = REPEATED[stage]
            return self._block(x, scope.format(k), stage, scale, True, training)
        if stage == "block8_last":
            return self._block(x, "Block8", "block8", 1.0, False, training)
        if stage == "conv_7b":
            return self._cbr(x, "Conv2d_7b_1x1", 1536, (1, 1), training)
        if stage == "head":
            return self._head(x, training)
        raise ValueError(f"unknown stage {stage!r}")

    def stages(self, x, stages, training, end_points=None):
        """A chain of stages; the k-th occurrence of a repeated stage is block k of its scope.  ``end_points``: filled with the
        output of every stage that is an end point of the model."""
        seen = {}
        for s in stages:
            seen[s] = seen.get(s, 0) + 1
            x = self.stage(x, s, training, seen[s])
            if end_points is not None and s in ("mixed_5a", "mixed_6a", "mixed_7a", "conv_7b"):
                end_points[{"conv_7b": "Conv2d_7b_1x1"}.get(s, s.capitalize())] = x
        return x

    def stem(self, images, training=False, preprocessed=False):
        x = images if preprocessed else fo.image_processing(images, 0, images.shape[1])
        x = _q(torch.as_tensor(x, dtype=torch.float32).permute(0, 3, 1, 2), self.dt)
        x = self._cbr(x, "Conv2d_1a_3x3", 32, (3, 3), training, 2, "valid")
        x = self._cbr(x, "Conv2d_2a_3x3", 32, (3, 3), training, 1, "valid")
        x = self._cbr(x, "Conv2d_2b_3x3", 64, (3, 3), training)
        x = self._maxpool(x)
        x = self._cbr(x, "Conv2d_3b_1x1", 80, (1, 1), training, 1, "valid")
        x = self._cbr(x, "Conv2d_4a_3x3", 192, (3, 3), training, 1, "valid")
        return self._maxpool(x)

    def model_stages(self):
        r35, r17, r8 = self.cfg["repeat"]
        return ["mixed_5a"] + ["block35"] * r35 + ["mixed_6a"] + ["block17"] * r17 + ["mixed_7a"] + ["block8"] * r8 + list(TAIL)

    def forward(self, images, training=False, preprocessed=False, end_points=None):
        ep = {}
        y = self.stages(self.stem(images, training, preprocessed), self.model_stages(), training, ep)
        ep["PreLogitsFlatten"] = self.pre_logits
        if end_points is not None:
            end_points.update(ep)
        return y


def train_step_grads(params, images, loss_kind, dt=None, keep=1.0, masks=None, labels=None, alpha=0.2, cfg=CFG):
    """(loss, {key: grad} of the trainable variables, embedding, new moving statistics)."""
    trainable = [k for k in params if not k.endswith(("moving_mean", "moving_variance"))]
    p = {k: (v.clone().requires_grad_(True) if k in trainable else v) for k, v in params.items()}
    o = IRv2(p, cfg=cfg, dt=dt, keep=keep, masks=masks)
    emb = o.forward(images, training=True)
    if loss_kind == "softmax":
        logits = _q(emb, dt) @ _q(p["classifier/logits/kernel"], dt) + p["classifier/logits/bias"]
        loss = fo.softmax_cross_entropy(logits, torch.as_tensor(labels))
    else:
        loss = fo.triplet_loss(fo.l2_normalize(emb), alpha)
    loss.backward()
    grads = {k: p[k].grad.detach().clone() if p[k].grad is not None else torch.zeros_like(p[k]) for k in trainable}
    return float(loss.detach()), grads, emb.detach(), o.new_stats


# ---- a lone stage or chain: the cases of tests/test_gpu_irv2_blocks.py and their rounded-autograd reference -------------------
# id -> (stages, input map H = W, input channels, N, keep).  Every BatchNorm sees >= 400 samples per channel (below that the
# comparison measures BatchNorm conditioning, not the kernels); the Bottleneck BN of the tails (N = 48) is the stated exception.
TAIL_STAGES = ("block8",) + TAIL
BLOCK_CASES = {
    "mixed_5a": (("mixed_5a",), 17, 192, 4, 1.0),
    "block35": (("block35",), 17, 320, 4, 1.0),
    "block35_x2": (("block35",) * 2, 17, 320, 4, 1.0),
    "mixed_6a": (("mixed_6a",), 17, 320, 8, 1.0),
    "block17": (("block17",), 8, 1088, 8, 1.0),
    "block17_x2": (("block17",) * 2, 8, 1088, 8, 1.0),
    "mixed_7a": (("mixed_7a",), 8, 1088, 48, 1.0),
    "block8": (("block8",), 3, 2080, 48, 1.0),
    "block8_x2": (("block8",) * 2, 3, 2080, 48, 1.0),
    "block8_last": (("block8_last",), 3, 2080, 48, 1.0),
    "chain_35_6a_17": (("block35", "mixed_6a", "block17"), 17, 320, 8, 1.0),
    "chain_17_7a_8": (("block17", "mixed_7a", "block8"), 8, 1088, 48, 1.0),
    "tail_keep_1": (TAIL_STAGES, 3, 2080, 48, 1.0),
    "tail_keep_half": (TAIL_STAGES, 3, 2080, 48, 0.5),
    "g299_mixed_5a": (("mixed_5a",), 35, 192, 2, 1.0),
    "g299_block35": (("block35",), 35, 320, 2, 1.0),
    "g299_mixed_6a": (("mixed_6a",), 35, 320, 2, 1.0),
    "g299_block17": (("block17",), 17, 1088, 2, 1.0),
    "g299_mixed_7a": (("mixed_7a",), 17, 1088, 8, 1.0),
    "g299_block8": (("block8",), 8, 2080, 8, 1.0),
    "g299_tail_keep_half": (TAIL_STAGES, 8, 2080, 48, 0.5),
}
BLOCK_SEED, BLOCK_E = 11, 128
TOL = {torch.float16: (1e-3, 2e-3), torch.bfloat16: (4e-3, 1e-2)}        # (tol_y, tol_g) of tests/test_gpu_blocks.py


def stages_out(stages, HW, Cc):
    """(map size, channels) after a chain of stages below ``head`` (default widths)."""
    for s in stages:
        if s in ("mixed_6a", "mixed_7a"):
            HW = (HW - 3) // 2 + 1
        Cc = {"mixed_5a": 320, "mixed_6a": 1088, "mixed_7a": 2080, "conv_7b": 1536}.get(s, Cc)
    return HW, Cc


def block_operands(net, case, dt):
    """(params, trainable keys, trunk NHWC in dt, incoming gradient, dropout mask or None) of a case: beta and bias are
    non-trivial, the trunk is relu(randn + 0.3) as after a ReLU of the real network, the incoming gradient is random (a random
    fp32 demb [N, E] after ``head``).  ``net``: the case's BlockNetworkV2 (allocated or not)."""
    stages, HW, Cc, N, keep = BLOCK_CASES[case]
    g = torch.Generator().manual_seed(5)
    params = net.init_keras_params(net.seed)              # what a freshly allocated network holds
    for k in params:
        if k.endswith("/beta") or k.endswith("/bias"):
            params[k] = 0.1 * torch.randn(params[k].shape, generator=g)
    trainable = [k for k in params if not k.endswith(("/moving_mean", "/moving_variance"))]
    x = torch.relu(torch.randn(N, HW, HW, Cc, generator=g) + 0.3).to(dt)
    if stages[-1] == "head":
        dout = 0.05 * torch.randn(N, net.E, generator=g)
    else:
        OH, Co = stages_out(stages, HW, Cc)
        dout = (0.05 * torch.randn(N, OH, OH, Co, generator=g)).to(dt)
    drop = dropout_mask(net.seed & 0xFFFFFFFF, 0, 0, N, 1536, keep) if keep < 1.0 else None
    return params, trainable, x, dout, drop


def block_reference(params, trainable, case, x, dout, dt, drop=None, relu_masks=None, pool_src=None, cls=None, x_nchw=None,
                    precision=torch.float32):
    """fp32 autograd through the case's stages on operands rounded where the HIP path stores them:
    (output NHWC or [N, E], dX NHWC, {key: gradient}, the restatement).  ``cls``: an IRv2 subclass (planted errors);
    ``precision``: torch.float64 evaluates the same rounded model (same parameters, same storage rounding) in fp64."""
    stages, HW, Cc, N, keep = BLOCK_CASES[case]
    if precision != torch.float32:
        params = {k: v.to(precision) for k, v in params.items()}
    for k in trainable:
        params[k].requires_grad_(True)
        params[k].grad = None
    o = (cls or IRv2)(params, dt=dt, keep=keep, masks=drop, relu_masks=relu_masks, pool_src=pool_src)
    xr = (x.to(precision).permute(0, 3, 1, 2).contiguous() if x_nchw is None else x_nchw).requires_grad_(True)
    y = o.stages(xr, stages, True)
    head = stages[-1] == "head"
    y.backward(dout.to(precision) if head else dout.to(precision).permute(0, 3, 1, 2))
    grads = {k: params[k].grad.detach().clone() for k in trainable if params[k].grad is not None}
    for k in trainable:
        params[k].requires_grad_(False)
        params[k].grad = None
    return (y.detach() if head else y.detach().permute(0, 2, 3, 1)), xr.grad.permute(0, 2, 3, 1), grads, o


# ---- the tail's bounds (Bottleneck BN over N = 48 samples) ----------------------------------------------------------------------
# Gradients.  Measured on the CPU against the reference alone (ulp_perturbed_distance below; tests/test_irv2_host.py repeats it):
# the trunk input moves by one storage ulp with random signs, the ReLU sets stay those of the unperturbed evaluation, and the
# distance is the largest relative L2 distance over dX and every dW / dbeta / dbias.  The bound is twice that, not below tol_g.
TAIL_MEASURED = {
    ("tail_keep_1", torch.float16): 1.83e-3, ("tail_keep_1", torch.bfloat16): 1.46e-2,
    ("tail_keep_half", torch.float16): 1.79e-3, ("tail_keep_half", torch.bfloat16): 1.43e-2,
    ("g299_tail_keep_half", torch.float16): 1.78e-3, ("g299_tail_keep_half", torch.bfloat16): 1.42e-2,
}
# Forward.  tol_y of tests/test_gpu_blocks.py for every case, with ONE measured exception: the tail without dropout in bf16.  The
# same rounded model (same parameters, same storage rounding) evaluated in fp64 lies 7.05e-3 from its own fp32 evaluation there
# (fp64_forward_distance below; tests/test_irv2_host.py repeats it; every other tail configuration: 3.7e-4 .. 9.7e-4 f16,
# 2.7e-3 / 4.0e-3 bf16, the stages and chains 6e-5 .. 1.6e-3): two correct evaluations of this case that differ only in summation
# order are further apart than 4e-3.  The bound of that case is four times the measured distance (another summation order again).
FP64_FORWARD = {("tail_keep_1", torch.bfloat16): 7.05e-3}
ZERO_BIAS = "Block8/Conv2d_1x1/bias"     # a constant per channel passes Conv2d_7b_1x1 (linear) and dies in its BatchNorm: the
#                                          gradient is zero in exact arithmetic, both sides hold rounding residue (~4e-6)


def tol_y(case, dt):
    """The forward bound of a case: tests/test_gpu_blocks.py's, or four times the measured fp64 distance of FP64_FORWARD."""
    m = FP64_FORWARD.get((case, dt))
    return TOL[dt][0] if m is None else 4 * m


def tol_g(case, dt):
    """The gradient bound of a case on shared sets: tests/test_gpu_blocks.py's, or the tail's measured one."""
    m = TAIL_MEASURED.get((case, dt))
    return TOL[dt][1] if m is None else max(2 * m, TOL[dt][1])


def fp64_forward_distance(net, case, dt):
    """Relative L2 distance between the fp32 and the fp64 evaluation of the case's rounded reference (forward)."""
    params, tr, x, dout, drop = block_operands(net, case, dt)
    y = block_reference(params, tr, case, x, dout, dt, drop)[0]
    return rel(y, block_reference(params, tr, case, x, dout, dt, drop, precision=torch.float64)[0])


def rel(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-30))


def ulp_perturbed_distance(net, case, dt, seed=99):
    """(forward, gradient) distance of the case's reference from itself with every non-zero trunk element moved by one ulp of dt."""
    params, tr, x, dout, drop = block_operands(net, case, dt)
    y, dx, g, o = block_reference(params, tr, case, x, dout, dt, drop)
    bits = x.view(torch.int16).clone()
    sign = torch.randint(0, 2, bits.shape, generator=torch.Generator().manual_seed(seed), dtype=torch.int16) * 2 - 1
    xp = torch.where(bits != 0, bits + sign, bits).view(dt)
    yp, dxp, gp, _ = block_reference(params, tr, case, xp, dout, dt, drop, relu_masks=o.own_relu)
    errs = [rel(gp[k], g[k]) for k in g if g[k].norm() > 1e-6 and k != ZERO_BIAS]
    return rel(yp, y), max(errs + [rel(dxp, dx)])
