"""Inception-ResNet-v2 on the static-plan engine (facenet/models/inception_resnet_v2.py:40-256 and its yaml).

The topology is lowered by the same ``Lowering`` as v1: stride-1 concat blocks (``Lowering.mixed``, whose Branch_3 opens with a
3x3 / stride 1 / SAME average pool: fn_avgpool3x3s1_*), the v1 reduction and residual-block code with v2's widths, and a head
that pools the whole final map and applies dropout to the pooled features in training (fn_dropout_*).  BatchNorm decays its
moving statistics with 0.995; the slim L2 regulariser (``weight_decay * sum(w^2) / 2``) is the Trainer's coupled
``g += 2 * l2 * w`` with ``l2 = weight_decay / 2``.

Variable names.  Engine layer names are the slim scope paths below ``InceptionResnetV2/``, so the checkpoint table is
``InceptionResnetV2/<layer>/weights`` (HWIO; ``[in, out]`` for ``Bottleneck``), ``.../biases`` (the residual ``Conv2d_1x1``) and
``.../BatchNorm/{beta,moving_mean,moving_variance}``.  The repeated blocks are scoped as ``tf_slim.repeat`` names them:
``Repeat/block35_<k>``, ``Repeat_1/block17_<k>``, ``Repeat_2/block8_<k>`` (k from 1), the unrepeated last block ``Block8``.
The softmax classifier of the training apps is ``Logits/{weights,biases}``, outside the model scope.  The table was derived
from tf_slim's scoping rules and has not been checked against a TensorFlow-written checkpoint (TensorFlow and tf_slim are not
available to this project's tests), so files are matched by name and the engine's own keys are accepted too.
"""
from __future__ import annotations

import copy
from collections import OrderedDict
from typing import Dict, List, Tuple

import torch

from .engine import Lowering, Network, towers

SCOPE = "InceptionResnetV2"
BN_MOMENTUM_V2 = 0.995          # inception_resnet_v2.py:232 (slim batch_norm decay)

DEFAULT_CONFIG_V2 = {           # models/configs/inception_resnet_v2.yaml
    "mixed_5a": {"branch": [[96], [48, 64], [64, 96, 96], [64]]},
    "mixed_6a": {"branch": [[384], [256, 256, 384]]},
    "mixed_7a": {"branch": [[256, 384], [256, 288], [256, 288, 320]]},
    "repeat": [10, 20, 9],
    "embedding_size": 512,
    "keep_probability": 0.5,
    "weight_decay": 0.0005,
}

# residual blocks (inception_resnet_v2.py:40-100): towers and the scale of `up`; up's width is the trunk's
V2_BLOCKS = {
    "block35": towers([("Conv2d_1x1", 32, (1, 1))],
                      [("Conv2d_0a_1x1", 32, (1, 1)), ("Conv2d_0b_3x3", 32, (3, 3))],
                      [("Conv2d_0a_1x1", 32, (1, 1)), ("Conv2d_0b_3x3", 48, (3, 3)), ("Conv2d_0c_3x3", 64, (3, 3))]),
    "block17": towers([("Conv2d_1x1", 192, (1, 1))],
                      [("Conv2d_0a_1x1", 128, (1, 1)), ("Conv2d_0b_1x7", 160, (1, 7)), ("Conv2d_0c_7x1", 192, (7, 1))]),
    "block8": towers([("Conv2d_1x1", 192, (1, 1))],
                     [("Conv2d_0a_1x1", 192, (1, 1)), ("Conv2d_0b_1x3", 224, (1, 3)), ("Conv2d_0c_3x1", 256, (3, 1))]),
}


def mixed_5a_towers(branch):
    b = branch
    return towers([("Conv2d_1x1", b[0][0], (1, 1))],
                  [("Conv2d_0a_1x1", b[1][0], (1, 1)), ("Conv2d_0b_5x5", b[1][1], (5, 5))],
                  [("Conv2d_0a_1x1", b[2][0], (1, 1)), ("Conv2d_0b_3x3", b[2][1], (3, 3)), ("Conv2d_0c_3x3", b[2][2], (3, 3))],
                  [("AvgPool_0a_3x3",), ("Conv2d_0b_1x1", b[3][0], (1, 1))])


def mixed_6a_towers(branch):
    b = branch
    return towers([("Conv2d_1a_3x3", b[0][0], (3, 3), 2, "valid")],
                  [("Conv2d_0a_1x1", b[1][0], (1, 1)), ("Conv2d_0b_3x3", b[1][1], (3, 3)), ("Conv2d_1a_3x3", b[1][2], (3, 3), 2, "valid")])


def mixed_7a_towers(branch):
    b = branch
    return towers([("Conv2d_0a_1x1", b[0][0], (1, 1)), ("Conv2d_1a_3x3", b[0][1], (3, 3), 2, "valid")],
                  [("Conv2d_0a_1x1", b[1][0], (1, 1)), ("Conv2d_1a_3x3", b[1][1], (3, 3), 2, "valid")],
                  [("Conv2d_0a_1x1", b[2][0], (1, 1)), ("Conv2d_0b_3x3", b[2][1], (3, 3)), ("Conv2d_1a_3x3", b[2][2], (3, 3), 2, "valid")])


def map_sizes(image_size: int) -> Tuple[int, int, int]:
    """Spatial size after Mixed_5a, Mixed_6a and Mixed_7a (17 / 8 / 3 at 160, 35 / 17 / 8 at 299)."""
    s = (image_size - 3) // 2 + 1           # Conv2d_1a_3x3 s2 VALID
    s = s - 2                               # Conv2d_2a_3x3 VALID (2b is SAME)
    s = (s - 3) // 2 + 1                    # MaxPool_3a
    s = s - 2                               # Conv2d_4a_3x3 VALID (3b is 1x1)
    s5 = (s - 3) // 2 + 1                   # MaxPool_5a
    s6 = (s5 - 3) // 2 + 1
    return s5, s6, (s6 - 3) // 2 + 1


# the stages after the stem, in the model's order: repeated residual stage -> (scope of block k, counted from 1; scale of `up`)
V2_REPEATED = {"block35": ("Repeat/block35_{}", 0.17), "block17": ("Repeat_1/block17_{}", 0.10), "block8": ("Repeat_2/block8_{}", 0.20)}
V2_TAIL = ("block8_last", "conv_7b", "head")        # Block8 (scale 1, no activation), Conv2d_7b_1x1, pool + dropout + Bottleneck
V2_STAGES = ("mixed_5a", "mixed_6a", "mixed_7a") + tuple(V2_REPEATED) + V2_TAIL


def lower_stages(g: Lowering, cfg, x, stages, E: int, keep: float):
    """The stages of Inception-ResNet-v2 below the stem (inception_resnet_v2.py:150-256), lowered in the given order onto the
    feature map ``x``: the whole model (NetworkV2._topology) and a lone stage or chain (BlockNetworkV2) go through these calls.
    The k-th occurrence of a repeated stage is block k of its ``tf_slim.repeat`` scope."""
    seen = {k: 0 for k in V2_REPEATED}
    for stage in stages:
        if stage == "mixed_5a":
            x = g.mixed("Mixed_5a", x, mixed_5a_towers(cfg["mixed_5a"]["branch"]))
        elif stage == "mixed_6a":
            x = g.reduction("Mixed_6a", x, mixed_6a_towers(cfg["mixed_6a"]["branch"]), branch="Branch_{}")
        elif stage == "mixed_7a":
            x = g.reduction("Mixed_7a", x, mixed_7a_towers(cfg["mixed_7a"]["branch"]), branch="Branch_{}")
        elif stage in V2_REPEATED:
            scope, scale = V2_REPEATED[stage]
            seen[stage] += 1
            x = g.block(scope.format(seen[stage]), x, V2_BLOCKS[stage], x.C, scale, True, branch="Branch_{}", up_name="Conv2d_1x1")
        elif stage == "block8_last":
            x = g.block("Block8", x, V2_BLOCKS["block8"], x.C, 1.0, False, branch="Branch_{}", up_name="Conv2d_1x1")
        elif stage == "conv_7b":
            x = g.cbr("Conv2d_7b_1x1", x, 1536, (1, 1), 1, "same")
        elif stage == "head":
            x = g.head(x, E, dense="Bottleneck", pool="Logits/AvgPool_1a", out="Bottleneck/bn", whole_map=True, keep=keep)
        else:
            raise ValueError(f"unknown Inception-ResNet-v2 stage {stage!r}: expected one of {V2_STAGES}")
    return x


class NetworkV2(Network):
    """Parameters + topology of Inception-ResNet-v2.  ``config``: the yaml's keys (``mixed_5a`` / ``mixed_6a`` / ``mixed_7a``
    ``.branch``, ``repeat``, ``embedding_size``, ``keep_probability``, ``weight_decay``); ``embedding_size`` given as an argument
    wins over the config's."""

    default_config = DEFAULT_CONFIG_V2
    bn_momentum = BN_MOMENTUM_V2

    def __init__(self, embedding_size=None, config=None, image_size: int = 160, **kw):
        cfg = copy.deepcopy(DEFAULT_CONFIG_V2)
        for k, v in (config or {}).items():
            cfg[k] = copy.deepcopy(v)
        E = int(cfg["embedding_size"] if embedding_size is None else embedding_size)
        cfg["embedding_size"] = E
        if min(map_sizes(int(image_size))) < 1:
            raise ValueError(f"Inception-ResNet-v2 needs images of at least 75 pixels (a 1x1 final map), got {image_size}")
        self.keep_probability = float(cfg["keep_probability"])
        if not 0.0 < self.keep_probability <= 1.0:
            raise ValueError(f"keep_probability must be in (0, 1], got {self.keep_probability}")
        self.l2_weight = float(cfg["weight_decay"]) / 2.0
        super().__init__(embedding_size=E, config=cfg, image_size=image_size, **kw)

    def _topology(self, g: Lowering):
        cfg = self.cfg
        s = self.image_size
        x = g.input(s, s)
        x = g.cbr("Conv2d_1a_3x3", x, 32, (3, 3), 2, "valid", cin_real=3)
        x = g.cbr("Conv2d_2a_3x3", x, 32, (3, 3), 1, "valid")
        x = g.cbr("Conv2d_2b_3x3", x, 64, (3, 3), 1, "same")
        x = g.maxpool("MaxPool_3a_3x3", x)
        x = g.cbr("Conv2d_3b_1x1", x, 80, (1, 1), 1, "valid")
        x = g.cbr("Conv2d_4a_3x3", x, 192, (3, 3), 1, "valid")
        x = g.maxpool("MaxPool_5a_3x3", x)
        r35, r17, r8 = (int(v) for v in cfg["repeat"])
        stages = ["mixed_5a"] + ["block35"] * r35 + ["mixed_6a"] + ["block17"] * r17 + ["mixed_7a"] + ["block8"] * r8 + list(V2_TAIL)
        return lower_stages(g, cfg, x, stages, self.E, self.keep_probability)

    # ---- slim variable names ------------------------------------------------------------------
    def variable_table(self) -> List[Tuple[str, str]]:
        """[(slim variable name, engine key)], layer by layer in declaration order."""
        out: List[Tuple[str, str]] = []
        for L in self.layers.values():
            scope = "Logits" if L.name == "classifier/logits" else f"{SCOPE}/{L.name}"
            out.append((f"{scope}/weights", L.name + "/kernel"))
            if L.has_bias:
                out.append((f"{scope}/biases", L.name + "/bias"))
            if L.has_bn:
                pre = self._bn_prefix(L)
                for v in ("beta", "moving_mean", "moving_variance"):
                    out.append((f"{scope}/BatchNorm/{v}", f"{pre}/{v}"))
        return out

    def _bn_prefix(self, L) -> str:
        return L.name + "/bn"

    def _engine_keys(self, params: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        out = {}
        table = self.variable_table()
        for k, i in table:
            for cand in (k, k + ":0", i):
                if cand in params:
                    out[i] = params[cand]
                    break
        missing = [k for k, i in table if i not in out]
        if missing:
            raise KeyError(f"weights file lacks {len(missing)} variables, first: {missing[0]}")
        return out

    def keras_variables(self, moving_stats=None, params=None) -> "OrderedDict[str, torch.Tensor]":
        """Every variable under its slim name (``variable_table`` order)."""
        p = self.export_keras_params(moving_stats, params)
        return OrderedDict((k, p[i]) for k, i in self.variable_table())


class BlockNetworkV2(NetworkV2):
    """A stage of Inception-ResNet-v2, or a chain of them (``stages``: names of V2_STAGES in the order they run; a chain may
    cross a reduction), on a [N,H,W,C] low-precision feature map: ``lower_stages`` on ``Lowering.feature_input``, so the lowering,
    the kernels and the fusions are those of the full network.  As with engine.BlockNetwork, ``plan.bufs['trunk']`` is the input
    (``.act`` in, ``.grad`` out) and ``plan.embedding`` the output of the last stage (``.act`` out, ``.grad`` in; after ``head``:
    the fp32 embedding, whose gradient ``build_backward`` takes)."""

    def __init__(self, stages, H: int, W: int, C: int, embedding_size: int = 128, config=None, **kw):
        self._stages = tuple([stages] if isinstance(stages, str) else stages)
        unknown = [s for s in self._stages if s not in V2_STAGES]
        if unknown or not self._stages:
            raise ValueError(f"unknown Inception-ResNet-v2 stages {unknown}: expected names of {V2_STAGES}")
        self._map = (int(H), int(W), int(C))
        super().__init__(embedding_size=embedding_size, config=config, **kw)

    def _topology(self, g: Lowering):
        return lower_stages(g, self.cfg, g.feature_input(*self._map), self._stages, self.E, self.keep_probability)

    def _engine_keys(self, params):
        return params          # a lone stage has no place in a checkpoint's variable naming: engine keys only


V1_MODULES = ("facenet.models.inception_resnet_v1", "facenet_amd.models.inception_resnet_v1")
V2_MODULES = ("facenet.models.inception_resnet_v2", "facenet_amd.models.inception_resnet_v2")


def network_class(module=None):
    """The engine network of a ``model.module`` name (apps/configs/train_softmax.yaml); v1 when none is given."""
    if not module or module in V1_MODULES:
        return Network
    if module in V2_MODULES:
        return NetworkV2
    raise ValueError(f"unknown model.module {module!r}: expected one of {V1_MODULES + V2_MODULES}")


def build_network(model_cfg, embedding_size: int, **kw) -> Network:
    """``model_cfg``: the app config's ``model`` section (``module``, optional ``config`` with the family's keys)."""
    cls = network_class(model_cfg.module if model_cfg else None)
    if cls is NetworkV2:
        sub = model_cfg.config
        return NetworkV2(embedding_size=embedding_size, config=sub.as_dict if sub else None, **kw)
    return Network(embedding_size=embedding_size, **kw)
