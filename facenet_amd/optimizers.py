"""The optimizer of a training step: the table of update rules behind ``train.optimizer``, the weights'
moving average that is fused into the update, and ``Optimizer``, which owns the state both keep on the
device, the launches that advance it and its part of a checkpoint."""
from __future__ import annotations

import warnings
from typing import Dict, List, NamedTuple, Optional, Tuple

import numpy as np
import torch

from . import _lib, keras_names
from .config import Config
from .engine import Network, _ptr
from .schedule import Op, emit, region


def adam_beta_powers(t: int, beta1: float, beta2: float) -> Tuple[float, float]:
    """(beta1^t, beta2^t) as fn_adam_tick derives them from the integer step count: the betas arrive on the device as fp32, the
    power is taken in double and rounded to fp32 once."""
    return float(np.float32(np.float64(np.float32(beta1)) ** t)), float(np.float32(np.float64(np.float32(beta2)) ** t))


def check_moving_average_decay(decay) -> Optional[float]:
    """The decay of the weights' moving average, or None when it is off (None or 0); anything outside (0, 1) raises."""
    if decay is None or decay == 0:
        return None
    d = float(decay)
    if not 0.0 < d < 1.0:
        raise ValueError(f"moving_average_decay must be in (0, 1), or None / 0 for off; got {decay!r}")
    return d


def moving_average_decay(cfg) -> Optional[float]:
    """``cfg.train.moving_average_decay`` (apps/configs/train_softmax.yaml:28) as the Trainer takes it: a missing key, null or
    0 is off (None)."""
    value = cfg.train.moving_average_decay
    return check_moving_average_decay(value if value else None)


class OptimizerRule(NamedTuple):
    """One value of train.optimizer: the Keras optimizer it maps to (its class name prefixes the checkpoint keys), the slot
    variables it keeps per parameter with their initial values, and the constants fn_opt_keras takes."""
    code: int                                   # fn_opt_keras rule code; 0: Adam (fn_adam_keras, the Trainer's beta1 / beta2 / epsilon)
    keras: str
    slots: Tuple[Tuple[str, float], ...]        # (Keras slot name, initial value)
    rho: float = 0.0
    momentum: float = 0.0
    epsilon: float = 0.0

    @property
    def op(self) -> str:
        """Name of the update launch in a step's schedule."""
        return f"{self.keras.lower()}_keras"


# The TF1 line's optimizer names (facenet.train) -> the Keras optimizers with the hyperparameters that line passes, as Adam's
# epsilon=0.1 carried over.  The only table of these constants.
OPTIMIZERS: Dict[str, OptimizerRule] = {
    "ADAGRAD": OptimizerRule(_lib.FN_OPT_ADAGRAD, "Adagrad", (("accumulator", 0.1),), epsilon=1e-7),
    "ADADELTA": OptimizerRule(_lib.FN_OPT_ADADELTA, "Adadelta", (("accum_grad", 0.0), ("accum_var", 0.0)), rho=0.9, epsilon=1e-6),
    "ADAM": OptimizerRule(0, "Adam", (("m", 0.0), ("v", 0.0))),
    "RMSPROP": OptimizerRule(_lib.FN_OPT_RMSPROP, "RMSprop", (("rms", 0.0), ("momentum", 0.0)), rho=0.9, momentum=0.9, epsilon=1.0),
    "MOM": OptimizerRule(_lib.FN_OPT_MOM, "SGD", (("momentum", 0.0),), momentum=0.9),
}


def check_optimizer(name) -> str:
    """A train.optimizer name; anything else raises the TF1 line's error."""
    if not isinstance(name, str) or name not in OPTIMIZERS:
        raise ValueError(f"Invalid optimization algorithm {name!r}: expected one of {', '.join(OPTIMIZERS)}")
    return name


def optimizer_name(cfg) -> str:
    """``cfg.train.optimizer`` (apps/configs/train_softmax.yaml:25-26) checked; a missing key or null is ADAM."""
    value = cfg.train.optimizer
    return check_optimizer("ADAM" if value is None or (isinstance(value, Config) and not value) else value)


def _trainable(net: Network):
    return [(k, i) for k, i in net.variable_table() if not i.endswith(("/moving_mean", "/moving_variance"))]


class Optimizer:
    """One update rule at work on ``net.P`` from the gradients ``G``: its slot variables, the device words ``hyper`` and, with
    ``ema_decay``, the moving average ``shadow`` of every trainable variable (all of P; not the moving statistics, not the
    centers), initialised from the weights every replica starts with; each replica applies the same update to the same reduced
    step, so neither is exchanged."""

    def __init__(self, net: Network, G: torch.Tensor, name: str, lr: float, beta1: float, beta2: float, epsilon: float, l2: float,
                 grad_scale: float, ema_decay: Optional[float], dt: int):
        self.net, self.G, self.name, self.rule = net, G, name, OPTIMIZERS[name]
        self.beta1, self.beta2, self.eps, self.l2, self.ema_decay, self.dt = beta1, beta2, epsilon, l2, ema_decay, dt      # beta1, beta2, epsilon: Adam's
        # the slot variables in the order of the OPTIMIZERS row, at their initial values
        self.slots: List[torch.Tensor] = [torch.full_like(G, init) for _, init in self.rule.slots]
        # hyper = {lr, beta1^t, beta2^t, grad_scale, t (int32 bits), 3 spare words}; lives on device so HIP-graph replays see
        # LR changes and advance Keras' step count themselves (fn_adam_tick: every rule; only Adam reads the beta powers)
        self.hyper = torch.tensor([lr, 1.0, 1.0, grad_scale, 0.0, 0.0, 0.0, 0.0], dtype=torch.float32, device=net.device)
        self.shadow: Optional[torch.Tensor] = None if ema_decay is None else net.P.clone()

    def ops(self) -> List[Op]:
        """Step count and beta powers (fn_adam_tick) -> the update rule in one pass over P, with the moving average fused in when
        it is kept -> the transposed pack."""
        net, lib, beta1, beta2, rule, ops = self.net, self.net.lib, self.beta1, self.beta2, self.rule, []
        emit(ops, "adam_tick", lib.fn_adam_tick, _ptr(self.hyper), beta1, beta2, w=[region(self.hyper)])
        opt_writes = [region(net.P)] + [region(s) for s in self.slots] + [region(net.W_train)]
        adam = self.name == "ADAM"
        # fn_adam_keras and fn_opt_keras are one pass of the same shape; fn_opt_keras takes its rule first, a one-slot rule no second slot
        fn, fn_ema = (lib.fn_adam_keras, lib.fn_adam_keras_ema) if adam else (lib.fn_opt_keras, lib.fn_opt_keras_ema)
        consts = (beta1, beta2, self.eps) if adam else (rule.rho, rule.momentum, rule.epsilon)
        opt_args = (() if adam else (rule.code,)) + (
            _ptr(net.P), _ptr(self.G), _ptr(self.slots[0]), _ptr(self.slots[1]) if len(self.slots) > 1 else None, _ptr(net.W_train),
            net.n_kernel, net.n_params, net.n_decay, _ptr(self.hyper), *consts, self.l2, self.dt)
        if self.shadow is None:
            emit(ops, rule.op, fn, *opt_args, r=[region(self.G), region(self.hyper)], w=opt_writes)
        else:      # the same launch with the moving-average update fused in (one pass, same launch count)
            emit(ops, rule.op + "_ema", fn_ema, *opt_args, _ptr(self.shadow), self.ema_decay,
                 r=[region(self.G), region(self.hyper)], w=opt_writes + [region(self.shadow)])
        emit(ops, "pack_transpose", lib.fn_pack_transpose, _ptr(net.W_train), _ptr(net.Wt_train), _ptr(net.table),
             len(net.layers), net.max_layer_elems, self.dt, r=[region(net.W_train)], w=[region(net.Wt_train)])
        return ops

    @property
    def iterations(self) -> int:
        """Keras' ``optimizer.iterations``: optimiser steps taken so far (an int32 word on the device, bumped by fn_adam_tick
        under every rule)."""
        return int(self.hyper.view(torch.int32)[4].item())

    @iterations.setter
    def iterations(self, t: int):
        """Sets the step count and the beta powers that belong to it (what the NEXT tick will overwrite with t + 1)."""
        if t < 0:
            raise ValueError(f"iteration count must be >= 0, got {t}")
        self.hyper.view(torch.int32)[4:5].fill_(int(t))
        self.hyper[1:3].copy_(torch.tensor(adam_beta_powers(t, self.beta1, self.beta2)))

    def reset(self, lr: Optional[float] = None):
        """The optimizer as freshly constructed: every slot at its initial value (Adam: zero moments; Adagrad: 0.1), t = 0."""
        for buf, (_, init) in zip(self.slots, self.rule.slots):
            buf.fill_(init)
        self.iterations = 0
        if lr is not None:
            self.set_learning_rate(lr)

    def set_learning_rate(self, lr: float):
        self.hyper[0:1].fill_(float(lr))     # device write: visible to the next graph replay

    # ---- checkpoints (apps/train_softmax.py:68-78,105; SURVEY.md section 5: optimiser state) -----------------------------
    def state_dict(self) -> Dict[str, np.ndarray]:
        """The Keras optimizer's slots ``<Optimizer>/<var>/<slot>`` (``Adam/<var>/m``, ``RMSprop/<var>/rms``, ...),
        ``<Optimizer>/iter`` and its learning rate."""
        net, out = self.net, {}
        table = dict((i, k) for k, i in net.variable_table())
        prefix, slot_names = self.rule.keras, tuple(s for s, _ in self.rule.slots)
        for j, buf in enumerate(self.slots):
            for key, t in net.export_keras_grads(buf).items():
                out[keras_names.optimizer_slot_names(table[key], prefix, slot_names)[j]] = t.numpy()
        out[f"{prefix}/iter:0"] = np.asarray(self.iterations, dtype=np.int64)
        out[f"{prefix}/learning_rate:0"] = np.asarray(self.hyper[0].item(), dtype=np.float32)
        return out

    def average_state_dict(self) -> Dict[str, np.ndarray]:
        """TF1's shadow variables, next to the optimizer's slots; nothing without a moving average."""
        if self.shadow is None:
            return {}
        table = dict((i, k) for k, i in self.net.variable_table())
        return {keras_names.moving_average_name(table[key]): t.numpy() for key, t in self.net.export_keras_grads(self.shadow).items()}

    def load_state_dict(self, sd: Dict[str, np.ndarray], path):
        """Restore slots, step count, learning rate and the moving average from the arrays of checkpoint ``path``, after the
        model variables.  A checkpoint written under another optimizer leaves this one fresh (Keras ``load_weights`` into a model
        compiled with another optimizer): initial slots, t = 0, this trainer's learning rate; a warning names both.  One without
        shadow variables restarts the average from the loaded weights."""
        net = self.net
        prefix, slot_names = self.rule.keras, tuple(s for s, _ in self.rule.slots)
        saved_by = [name for name, r in OPTIMIZERS.items() if f"{r.keras}/iter:0" in sd]
        if f"{prefix}/iter:0" in sd:
            for slot, (buf, (_, init)) in enumerate(zip(self.slots, self.rule.slots)):
                tmp = {i: torch.from_numpy(sd[keras_names.optimizer_slot_names(k, prefix, slot_names)[slot]]) for k, i in _trainable(net)}
                flat = net.flat_from_keras(tmp)
                if init != 0:      # the channel padding has no Keras value: it keeps the slot's initial value, as in a fresh trainer
                    real = net.flat_from_keras({i: torch.ones_like(t) for i, t in tmp.items()}) != 0
                    flat = torch.where(real, flat, torch.full_like(flat, init))
                buf.copy_(flat)
            self.hyper[0:1].fill_(float(sd[f"{prefix}/learning_rate:0"]))
            self.iterations = int(sd[f"{prefix}/iter:0"])
        elif saved_by:
            warnings.warn(f"checkpoint {path} holds {saved_by[0]} optimizer state but this trainer's optimizer is {self.name}: "
                          f"the model variables are restored and the {self.name} state starts fresh")
            self.reset()
        if self.shadow is not None:
            trainable = _trainable(net)
            if keras_names.moving_average_name(trainable[0][0]) in sd:
                self.shadow.copy_(net.flat_from_keras({i: torch.from_numpy(sd[keras_names.moving_average_name(k)]) for k, i in trainable}))
            else:                                               # a checkpoint of a run without the moving average
                self.shadow.copy_(net.P)
