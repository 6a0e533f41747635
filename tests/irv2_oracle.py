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
    return x if dt is None else x + (x.to(dt).to(torch.float32) - x).detach()


def param_names(E=128, nrof_classes=None, cfg=CFG):
    """Engine keys of every variable the restatement reads, in declaration order."""
    return list(IRv2(None, cfg=cfg).declare(E, nrof_classes))


class IRv2:
    def __init__(self, params, cfg=CFG, dt=None, keep=1.0, masks=None):
        self.p, self.cfg, self.dt, self.keep, self.masks = params, cfg, dt, keep, masks
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

    def _bn(self, y, name, training, relu=True):
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
        z = (_q(y, self.dt) - mean.view(1, -1, 1, 1)) * torch.rsqrt(var.view(1, -1, 1, 1) + BN_EPS) + beta.view(1, -1, 1, 1)
        return _q(F.relu(z) if relu else z, self.dt)

    def _cbr(self, x, name, cout, k, training, stride=1, padding="same"):
        return self._bn(self._conv(x, name, k, stride, padding, cout=cout), name, training)

    def _maxpool(self, x):
        return F.max_pool2d(x, 3, 2)

    def _towers(self, x, pre, towers, training):
        outs = []
        for i, t in enumerate(towers):
            y = x
            for spec in t:
                if spec[0].startswith("AvgPool"):
                    y = _q(F.avg_pool2d(y, 3, 1, 1, count_include_pad=False), self.dt)
                    continue
                nm, cout, k = spec[:3]
                stride, padding = (spec[3], spec[4]) if len(spec) > 3 else (1, "same")
                y = self._cbr(y, f"{pre}/Branch_{i}/{nm}", cout, k, training, stride, padding)
            outs.append(y)
        return outs

    def _block(self, x, pre, kind, scale, relu, training):
        from facenet_amd.engine_v2 import V2_BLOCKS
        mixed = torch.cat(self._towers(x, pre, V2_BLOCKS[kind], training), 1)
        up = self._conv(mixed, pre + "/Conv2d_1x1", (1, 1), bias=True, cout=x.shape[1])
        y = x + scale * up
        return _q(F.relu(y) if relu else y, self.dt)

    def forward(self, images, training=False, preprocessed=False, end_points=None):
        from facenet_amd import engine_v2 as v2
        cfg = self.cfg
        x = images if preprocessed else fo.image_processing(images, 0, images.shape[1])
        x = _q(torch.as_tensor(x, dtype=torch.float32).permute(0, 3, 1, 2), self.dt)
        x = self._cbr(x, "Conv2d_1a_3x3", 32, (3, 3), training, 2, "valid")
        x = self._cbr(x, "Conv2d_2a_3x3", 32, (3, 3), training, 1, "valid")
        x = self._cbr(x, "Conv2d_2b_3x3", 64, (3, 3), training)
        x = self._maxpool(x)
        x = self._cbr(x, "Conv2d_3b_1x1", 80, (1, 1), training, 1, "valid")
        x = self._cbr(x, "Conv2d_4a_3x3", 192, (3, 3), training, 1, "valid")
        x = self._maxpool(x)
        x = torch.cat(self._towers(x, "Mixed_5a", v2.mixed_5a_towers(cfg["mixed_5a"]), training), 1)
        ep = {"Mixed_5a": x}
        for i in range(cfg["repeat"][0]):
            x = self._block(x, f"Repeat/block35_{i + 1}", "block35", 0.17, True, training)
        x = torch.cat(self._towers(x, "Mixed_6a", v2.mixed_6a_towers(cfg["mixed_6a"]), training) + [self._maxpool(x)], 1)
        ep["Mixed_6a"] = x
        for i in range(cfg["repeat"][1]):
            x = self._block(x, f"Repeat_1/block17_{i + 1}", "block17", 0.10, True, training)
        x = torch.cat(self._towers(x, "Mixed_7a", v2.mixed_7a_towers(cfg["mixed_7a"]), training) + [self._maxpool(x)], 1)
        ep["Mixed_7a"] = x
        for i in range(cfg["repeat"][2]):
            x = self._block(x, f"Repeat_2/block8_{i + 1}", "block8", 0.20, True, training)
        x = self._block(x, "Block8", "block8", 1.0, False, training)
        x = self._cbr(x, "Conv2d_7b_1x1", 1536, (1, 1), training)
        ep["Conv2d_7b_1x1"] = x
        x = _q(x.mean(dim=(2, 3)), self.dt)                       # AvgPool_1a over the whole map + flatten
        if training and self.keep < 1.0:
            x = _q(x * torch.as_tensor(self.masks, dtype=torch.float32) / self.keep, self.dt)
        ep["PreLogitsFlatten"] = x
        w = self._get("Bottleneck/kernel")
        if self._names is not None:
            y = torch.zeros(x.shape[0], self.E, 1, 1)
        else:
            y = (x @ _q(w, self.dt)).view(x.shape[0], -1, 1, 1)
        y = self._bn(y, "Bottleneck", training, relu=False).view(x.shape[0], -1)
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
