"""``InceptionResnetV2`` with v1's call contract (facenet/models/inception_resnet_v2.py:40-256): ``InceptionResnetV2(input_shape,
image_processing, config=None)``; ``model(inputs, training=False) -> float32 [N,E]`` (L2-normalised when ``training`` is False);
plans cached per batch size, inference replayed as one HIP graph.  ``inference(images, config, phase_train)`` returns the
reference's ``(bottleneck, end_points)``.  The network itself is engine_v2.NetworkV2."""
from __future__ import annotations

from typing import Dict

import numpy as np
import torch

from ..config import Config
from ..engine_v2 import DEFAULT_CONFIG_V2, NetworkV2
from .inception_resnet_v1 import InceptionResnetV1

default_model_config = Config(DEFAULT_CONFIG_V2)
default_config = default_model_config


def check_input_config(cfg=None):
    return Config(DEFAULT_CONFIG_V2) if cfg is None else cfg


class InceptionResnetV2(InceptionResnetV1):
    def __init__(self, input_shape, image_processing, config=None, device: str = "cuda", seed: int = 0,
                 infer_dtype: torch.dtype = torch.float16, train_dtype: torch.dtype = torch.bfloat16, nrof_classes=None):
        self.config = check_input_config(config)
        self.image_processing = image_processing
        cfg = self.config.as_dict if isinstance(self.config, Config) else dict(self.config)
        size = int(input_shape[0]) if input_shape is not None else image_processing.config.size
        norm = image_processing.config.normalization if image_processing is not None else 0
        self.network = NetworkV2(config=cfg, image_size=size, normalization=int(norm), nrof_classes=nrof_classes, device=device,
                                 train_dtype=train_dtype, infer_dtype=infer_dtype, seed=seed)
        self.custom_layers = ("Conv2d_1a_3x3", "Mixed_5a", "Repeat", "Mixed_6a", "Repeat_1", "Mixed_7a", "Repeat_2", "Block8",
                              "Conv2d_7b_1x1", "Logits", "Bottleneck")
        self._plans: Dict[tuple, object] = {}
        self._f32_in: Dict[int, torch.Tensor] = {}
        self._graphs: Dict[int, tuple] = {}

    def __call__(self, inputs, training: bool = False, **kwargs) -> torch.Tensor:
        out = super().__call__(inputs, training=training, **kwargs)
        if training:
            plan = self._plans.get((int(out.shape[0]), True))
            if plan is not None and plan.step_word is not None:
                plan.step_word.add_(1)          # the plan's own dropout step: the next training call draws new masks
        return out

    def end_points(self, n: int, training: bool) -> Dict[str, torch.Tensor]:
        """Activations of the last forward of the batch-``n`` plan (NHWC, float32 copies)."""
        plan = self._plan(n, training)
        E = self.network.E
        ep = {k: plan.bufs[b].act.float().clone() for k, b in (("Mixed_5a", "Mixed_5a/out"), ("Mixed_6a", "Mixed_6a/out"),
                                                              ("Mixed_7a", "Mixed_7a/out"), ("Conv2d_7b_1x1", "Conv2d_7b_1x1"))}
        ep["PreLogitsFlatten"] = plan.pre_logits.act.float().reshape(n, -1).clone()
        ep["Bottleneck"] = plan.embedding.buf.act.view(n, E).clone()
        return ep


_models: Dict[tuple, InceptionResnetV2] = {}


def inference(images, config=None, phase_train: bool = True, device: str = "cuda"):
    """(bottleneck [N,E] un-normalised, end_points) for NHWC uint8 / float images; models are cached per (config, size)."""
    x = torch.as_tensor(np.asarray(images)) if not torch.is_tensor(images) else images
    cfg = check_input_config(config)
    key = (repr(cfg), int(x.shape[1]), device)
    if key not in _models:
        _models[key] = InceptionResnetV2((int(x.shape[1]), int(x.shape[2]), 3), None, cfg, device=device)
    model = _models[key]
    n = int(x.shape[0])
    if phase_train:
        emb = model(x, training=True)
    else:
        model(x, training=False)
        emb = model._plan(n, False).embedding.buf.act.view(n, -1).clone()
    return emb, model.end_points(n, phase_train)
