"""Host-side description of a network's variables: the layer table, the flat parameter layout and its Keras-layout import / export.

Parameters, gradients and optimizer slots are single flat fp32 buffers laid out ``[kernels OHWI | pad | betas | biases]``; the
kernels are padded to 8 input channels (and the classifier to 8 output rows), Keras keeps them un-padded as HWIO (``[in, out]`` for
dense layers).  ``pack`` and ``unpack`` are the only code that converts between the two (apps/train_softmax.py:68-78 is what reads
and writes the Keras side).  Nothing here touches the device or the compiled library.
"""
from __future__ import annotations

import math
from collections import OrderedDict
from dataclasses import dataclass
from typing import Callable, Dict, Iterable, Optional, Tuple

import torch


def _pad8(c: int) -> int:
    return (c + 7) // 8 * 8


@dataclass
class Layer:
    name: str
    cin: int          # padded to a multiple of 8
    cin_real: int
    cout: int
    kh: int
    kw: int
    stride: int
    pad_h: int
    pad_w: int
    has_bn: bool
    has_bias: bool
    dense: bool = False
    cout_real: int = -1   # un-padded output channels (classifier only differs)
    w_off: int = -1       # element offset of [cout][kh][kw][cin] in the flat parameter buffer
    bias_off: int = -1    # element offset of the bias in the flat parameter buffer
    bn_off: int = -1      # offset in the global BatchNorm channel space
    index: int = -1

    @property
    def ktot(self) -> int:
        return self.kh * self.kw * self.cin

    @property
    def numel(self) -> int:
        return self.cout * self.ktot


def _layout(layers: Iterable[Layer], CB: int) -> Tuple[int, int, int]:
    """Assign ``w_off`` / ``bias_off`` of every layer of the flat buffer [kernels | pad | CB betas | biases | pad].
    -> (n_kernel, n_decay: the betas' offset, n_params)"""
    layers = list(layers)
    off = 0
    for L in layers:
        L.w_off = off
        off += L.numel
        assert L.numel % 8 == 0
    n_kernel = off
    n_decay = (off + 3) // 4 * 4            # coupled-L2 region of the flat buffer
    off = n_decay + CB
    for L in layers:
        if L.has_bias:
            L.bias_off = off
            off += L.cout
    return n_kernel, n_decay, (off + 3) // 4 * 4


def count_variables(layers: Iterable[Layer]) -> Tuple[int, int]:
    """(total, trainable) counted on the UN-padded Keras shapes (SURVEY.md shape table)."""
    tot = tr = 0
    for L in layers:
        k = L.cout_real * L.kh * L.kw * L.cin_real
        tr += k + (L.cout_real if L.has_bias else 0) + (L.cout if L.has_bn else 0)
        tot += k + (L.cout_real if L.has_bias else 0) + (3 * L.cout if L.has_bn else 0)
    return tot, tr


def init_keras_params(layers: Iterable[Layer], bn_prefix: Callable[[Layer], str], seed: int = 0) -> "OrderedDict[str, torch.Tensor]":
    """Glorot-uniform kernels (inception_resnet_v1.py:66), zero biases / beta, moving stats (0, 1),
    drawn in declaration order from torch.Generator(seed) on the CPU."""
    gen = torch.Generator().manual_seed(seed)
    out: "OrderedDict[str, torch.Tensor]" = OrderedDict()
    for L in layers:
        if L.dense:
            w = torch.empty(L.cin_real, L.cout_real)
            lim = math.sqrt(6.0 / (L.cin_real + L.cout_real))
        else:
            w = torch.empty(L.kh, L.kw, L.cin_real, L.cout)
            lim = math.sqrt(6.0 / (L.kh * L.kw * (L.cin_real + L.cout)))
        w.uniform_(-lim, lim, generator=gen)
        out[L.name + "/kernel"] = w
        if L.has_bias:
            out[L.name + "/bias"] = torch.zeros(L.cout_real)
        if L.has_bn:
            pre = bn_prefix(L)
            out[pre + "/beta"] = torch.zeros(L.cout)
            out[pre + "/moving_mean"] = torch.zeros(L.cout)
            out[pre + "/moving_variance"] = torch.ones(L.cout)
    return out


def kernel_from_keras(L: Layer, w) -> torch.Tensor:
    """A Keras kernel (HWIO; [in, out] for a dense layer) as the padded [cout][kh][kw][cin] block of the flat buffer."""
    w = torch.as_tensor(w).to(torch.float32)
    if L.dense:
        w = w.t().reshape(L.cout_real, 1, 1, L.cin_real)
        if L.cout != L.cout_real:
            w = torch.cat([w, torch.zeros(L.cout - L.cout_real, 1, 1, L.cin_real)], 0)
    else:
        w = w.permute(3, 0, 1, 2)                      # HWIO -> O,H,W,I
    if L.cin != L.cin_real:
        w = torch.nn.functional.pad(w, (0, L.cin - L.cin_real))
    return w.reshape(-1)


def kernel_to_keras(L: Layer, flat: torch.Tensor) -> torch.Tensor:
    """The inverse: layer L's block of a flat (host) buffer, padding dropped, in the Keras layout."""
    w = flat[L.w_off:L.w_off + L.numel].reshape(L.cout, L.kh, L.kw, L.cin)[:L.cout_real, ..., :L.cin_real]
    return (w.reshape(L.cout_real, L.cin_real).t() if L.dense else w.permute(1, 2, 3, 0)).contiguous()


def pack(layers: Iterable[Layer], n_params: int, beta_base: int, CB: int, bn_prefix: Callable[[Layer], str],
         params: Dict[str, torch.Tensor], with_stats: bool):
    """Engine-keyed Keras-layout tensors -> the flat fp32 layout (+ moving statistics, (0, 1) unless ``with_stats``)."""
    P = torch.zeros(n_params, dtype=torch.float32)
    mean, var = torch.zeros(CB), torch.ones(CB)
    for L in layers:
        P[L.w_off:L.w_off + L.numel] = kernel_from_keras(L, params[L.name + "/kernel"])
        if L.has_bias:
            P[L.bias_off:L.bias_off + L.cout_real] = torch.as_tensor(params[L.name + "/bias"]).to(torch.float32)
        if L.has_bn:
            pre, bn = bn_prefix(L), slice(L.bn_off, L.bn_off + L.cout)
            P[beta_base + bn.start:beta_base + bn.stop] = torch.as_tensor(params[pre + "/beta"])
            if with_stats:
                mean[bn] = torch.as_tensor(params[pre + "/moving_mean"])
                var[bn] = torch.as_tensor(params[pre + "/moving_variance"])
    return P, mean, var


def unpack(layers: Iterable[Layer], beta_base: int, bn_prefix: Callable[[Layer], str], flat: torch.Tensor,
           stats: Optional[Tuple[torch.Tensor, torch.Tensor]] = None) -> "OrderedDict[str, torch.Tensor]":
    """A flat host buffer laid out like ``P`` -> Keras-layout tensors under the engine's keys: per layer kernel, bias, beta and,
    given ``stats`` = (mean, var) over the BatchNorm channel space, the moving statistics."""
    out: "OrderedDict[str, torch.Tensor]" = OrderedDict()
    for L in layers:
        out[L.name + "/kernel"] = kernel_to_keras(L, flat)
        if L.has_bias:
            out[L.name + "/bias"] = flat[L.bias_off:L.bias_off + L.cout_real].clone()
        if L.has_bn:
            pre, bn = bn_prefix(L), slice(L.bn_off, L.bn_off + L.cout)
            out[pre + "/beta"] = flat[beta_base + bn.start:beta_base + bn.stop].clone()
            if stats is not None:
                out[pre + "/moving_mean"] = stats[0][bn].clone()
                out[pre + "/moving_variance"] = stats[1][bn].clone()
    return out
