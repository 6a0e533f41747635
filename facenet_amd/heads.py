"""The loss heads of a training step: what runs between the network's forward and its backward, from the embedding to its
gradient ``demb``.

* ``triplet_head``: l2_normalize -> triplet loss over rows (a0,p0,n0,a1,...) (arXiv 1503.03832).
* ``batch_triplet_head``: l2_normalize -> squared distances -> batch-hard / batch-all triplet loss mined inside the labelled batch
  (arXiv 1703.07737 sec. 2).
* ``xbm_triplet_head``: batch hard mined over the batch and a cross-batch memory of earlier steps' rows (Wang et al., CVPR 2020;
  DESIGN.md section 32).
* ``softmax_head``: the classifier Dense(C) + softmax cross-entropy (apps/train_softmax.py:49-104), or with ``margin`` the
  large-margin cosine softmax (NormFace / CosFace / ArcFace) through the same classifier launches.
* ``add_regularizers``: center loss and prelogits norm on a softmax head (facenet/facenet.py:204-217).

A head is plain data (``Head``): the Trainer splices its launches into the step and exposes its tensors as attributes."""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from . import _lib
from .engine import Network, _ptr, bias_region, weight_region
from .schedule import Op, emit, region, torch_op


XBM_MAX_ROWS = 65536                                          # the rows fn_xbm_triplet_fwd_bwd takes as a memory
TRIPLET_STRATEGIES = ("mined", "batch_hard", "batch_all")      # "mined": TripletMiner fills the (a,p,n) rows; the others: fn_batch_triplet_fwd_bwd


def check_loss_arguments(net: Network, batch: int, loss: str, center_factor: float, center_alfa: float, prelogits_norm_factor: float,
                         prelogits_norm_p: float, margin_scale: float = 0.0, margin_arc: float = 0.0, margin_cos: float = 0.0,
                         triplet_strategy: str = "mined", soft_margin: bool = False, memory_size: int = 0, memory_start: int = 0):
    """What the Trainer refuses: an unknown loss, a batch or network that does not fit it, regulariser settings out of range
    (loss.center_factor / center_alfa / prelogits_norm_factor / prelogits_norm_p, train_softmax.yaml:73-78), margin settings out of
    range or without a scale (loss.margin_scale / margin_arc / margin_cos), an unknown triplet strategy or
    one that does not fit the loss or the batch (loss.triplet_strategy / soft_margin), a cross-batch memory
    without batch hard, smaller than the batch or larger than 65 536 rows (loss.memory_size / memory_start)."""
    if loss not in ("triplet", "softmax"):
        raise ValueError(f"unknown loss {loss!r}")
    if triplet_strategy not in TRIPLET_STRATEGIES:
        raise ValueError(f"unknown triplet_strategy {triplet_strategy!r}: expected one of {', '.join(TRIPLET_STRATEGIES)}")
    if loss == "softmax" and (triplet_strategy != "mined" or soft_margin):
        raise ValueError("triplet_strategy and soft_margin belong to triplet training")
    if soft_margin and triplet_strategy == "mined":
        raise ValueError("soft_margin needs triplet_strategy 'batch_hard' or 'batch_all': the mined triplet loss has the hinge only")
    if batch < 2:
        raise ValueError(f"batch must be >= 2, got {batch}")
    if loss == "triplet" and triplet_strategy == "mined" and batch % 3:
        raise ValueError("triplet batches are laid out (a,p,n,...): batch must be a multiple of 3")
    if loss == "triplet" and triplet_strategy != "mined" and batch > 1024:
        raise ValueError(f"the batch-mined triplet losses take at most 1024 rows, got batch {batch}")
    if isinstance(memory_size, bool) or not isinstance(memory_size, (int, np.integer)) or memory_size < 0:
        raise ValueError(f"memory_size must be a non-negative integer, got {memory_size!r}")
    if isinstance(memory_start, bool) or not isinstance(memory_start, (int, np.integer)) or memory_start < 0:
        raise ValueError(f"memory_start must be a non-negative integer, got {memory_start!r}")
    if memory_size and (loss != "triplet" or triplet_strategy != "batch_hard"):
        raise ValueError("the cross-batch memory needs loss 'triplet' with triplet_strategy 'batch_hard'")
    if memory_size and not batch <= memory_size <= XBM_MAX_ROWS:
        raise ValueError(f"memory_size must be in [batch, {XBM_MAX_ROWS}] = [{batch}, {XBM_MAX_ROWS}], got {memory_size}")
    if loss == "softmax" and net.nrof_classes is None:
        raise ValueError("softmax training needs Network(nrof_classes=...)")
    if not (center_factor >= 0 and prelogits_norm_factor >= 0):
        raise ValueError(f"center_factor and prelogits_norm_factor must be >= 0, got {center_factor}, {prelogits_norm_factor}")
    if not 0 <= center_alfa <= 1:
        raise ValueError(f"center_alfa must be in [0, 1], got {center_alfa}")
    if not prelogits_norm_p > 0:
        raise ValueError(f"prelogits_norm_p must be > 0, got {prelogits_norm_p}")
    if loss == "triplet" and (center_factor > 0 or prelogits_norm_factor > 0):
        raise ValueError("center loss and prelogits-norm loss need class labels: they belong to softmax training")
    if not (margin_scale >= 0 and margin_arc >= 0 and margin_cos >= 0):
        raise ValueError(f"margin_scale, margin_arc and margin_cos must be >= 0, got {margin_scale}, {margin_arc}, {margin_cos}")
    if not float(np.float32(margin_arc)) < math.pi / 2:      # the kernel takes the fp32 value
        raise ValueError(f"margin_arc must be < pi/2, got {margin_arc}")
    if margin_scale == 0 and (margin_arc > 0 or margin_cos > 0):
        raise ValueError("margin_arc and margin_cos need margin_scale > 0")
    if loss == "triplet" and margin_scale > 0:
        raise ValueError("the margin softmax needs class labels: it belongs to softmax training")


@dataclass
class Head:
    """What a loss head hands the Trainer."""
    loss_ops: List[Op] = field(default_factory=list)         # after the forward: the loss and the embedding's gradient
    tensors: Dict[str, torch.Tensor] = field(default_factory=dict)      # every tensor its launches point at, by Trainer attribute
    pre_ops: List[Op] = field(default_factory=list)          # before the forward
    final_ops: List[Op] = field(default_factory=list)        # the final segment, after the optimizer
    state: Tuple[str, ...] = ()                              # the tensors a step mutates and the next step reads
    keep: tuple = ()                                         # what a launch points at that no Op.keep holds


def triplet_head(net: Network, emb: torch.Tensor, demb: torch.Tensor, loss: torch.Tensor, alpha: float) -> Head:
    """l2_normalize -> triplet loss over rows (a0,p0,n0,a1,...) -> gradient wrt the un-normalised embedding (demb)."""
    lib, (batch, E) = net.lib, emb.shape
    embn = torch.zeros(batch, E, dtype=torch.float32, device=net.device)
    dembn = torch.zeros(batch, E, dtype=torch.float32, device=net.device)
    ops: List[Op] = []
    emit(ops, "l2norm_fwd", lib.fn_l2norm_fwd, _ptr(emb), _ptr(embn), batch, E, 1e-10, r=[region(emb)], w=[region(embn)])
    emit(ops, "triplet_loss", lib.fn_triplet_loss_fwd_bwd, _ptr(embn), _ptr(dembn), _ptr(loss),
         batch // 3, E, alpha, r=[region(embn)], w=[region(dembn), region(loss)])
    emit(ops, "l2norm_bwd", lib.fn_l2norm_bwd, _ptr(emb), _ptr(dembn), _ptr(demb), batch, E, 1e-10,
         r=[region(emb), region(dembn)], w=[region(demb)])
    return Head(ops, dict(embn=embn, dembn=dembn))


def batch_triplet_head(net: Network, emb: torch.Tensor, demb: torch.Tensor, loss: torch.Tensor, alpha: float, strategy: str,
                       soft: bool) -> Head:
    """l2_normalize -> [batch,batch] squared distances -> batch-hard / batch-all loss mined inside the labelled batch -> gradient wrt
    the un-normalised embedding.  ``labels`` (int32 [batch], on the device) name the identities; the head
    carries nothing from step to step."""
    lib, dev, (batch, E) = net.lib, net.device, emb.shape
    embn = torch.zeros(batch, E, dtype=torch.float32, device=dev)
    dembn = torch.zeros(batch, E, dtype=torch.float32, device=dev)
    dist = torch.zeros(batch, batch, dtype=torch.float32, device=dev)
    coef = torch.zeros(batch, batch, dtype=torch.float32, device=dev)
    labels = torch.zeros(batch, dtype=torch.int32, device=dev)
    mine_info = torch.zeros(8, dtype=torch.int32, device=dev)
    ops: List[Op] = []
    emit(ops, "l2norm_fwd", lib.fn_l2norm_fwd, _ptr(emb), _ptr(embn), batch, E, 1e-10, r=[region(emb)], w=[region(embn)])
    emit(ops, "pairwise_sqdist", lib.fn_pairwise_sqdist, _ptr(embn), _ptr(embn), _ptr(dist), None, batch, batch, E, 2,
         r=[region(embn)], w=[region(dist)])
    emit(ops, "batch_triplet", lib.fn_batch_triplet_fwd_bwd, _ptr(embn), _ptr(dist), _ptr(labels), _ptr(dembn), _ptr(loss), _ptr(coef),
         _ptr(mine_info), batch, E, alpha, TRIPLET_STRATEGIES.index(strategy) - 1, 1 if soft else 0,
         r=[region(embn), region(dist), region(labels)], w=[region(dembn), region(loss), region(coef), region(mine_info)])
    emit(ops, "l2norm_bwd", lib.fn_l2norm_bwd, _ptr(emb), _ptr(dembn), _ptr(demb), batch, E, 1e-10,
         r=[region(emb), region(dembn)], w=[region(demb)])
    return Head(ops, dict(embn=embn, dembn=dembn, dist=dist, coef=coef, labels=labels, mine_info=mine_info))


def xbm_triplet_head(net: Network, emb: torch.Tensor, demb: torch.Tensor, loss: torch.Tensor, alpha: float, soft: bool,
                     memory_size: int, memory_start: int) -> Head:
    """batch_triplet_head's batch hard with a cross-batch memory: the anchors are mined over the batch and a ring
    of the last ``memory_size`` normalised rows of earlier steps.  The enqueue comes last, so a step never mines against its own rows;
    the ring (mem_emb, mem_labels, mem_state) is the head's state.  ``labels`` must name the same identity in every step."""
    lib, dev, (batch, E), M = net.lib, net.device, emb.shape, memory_size
    f32 = dict(dtype=torch.float32, device=dev)
    i32 = dict(dtype=torch.int32, device=dev)
    embn, dembn = torch.zeros(batch, E, **f32), torch.zeros(batch, E, **f32)
    dist, coef = torch.zeros(batch, batch, **f32), torch.zeros(batch, batch, **f32)
    labels, mine_info = torch.zeros(batch, **i32), torch.zeros(8, **i32)
    mem_emb, mem_labels, mem_state = torch.zeros(M, E, **f32), torch.zeros(M, **i32), torch.zeros(4, **i32)
    mem_dist, mpick, mcoef = torch.zeros(batch, M, **f32), torch.zeros(batch, 2, **i32), torch.zeros(batch, 2, **f32)
    ring = [region(mem_emb), region(mem_labels), region(mem_state)]
    ops: List[Op] = []
    emit(ops, "l2norm_fwd", lib.fn_l2norm_fwd, _ptr(emb), _ptr(embn), batch, E, 1e-10, r=[region(emb)], w=[region(embn)])
    emit(ops, "pairwise_sqdist", lib.fn_pairwise_sqdist, _ptr(embn), _ptr(embn), _ptr(dist), None, batch, batch, E, 2,
         r=[region(embn)], w=[region(dist)])
    emit(ops, "pairwise_sqdist", lib.fn_pairwise_sqdist, _ptr(embn), _ptr(mem_emb), _ptr(mem_dist), None, batch, M, E, 2,
         r=[region(embn), region(mem_emb)], w=[region(mem_dist)])
    emit(ops, "xbm_triplet", lib.fn_xbm_triplet_fwd_bwd, _ptr(embn), _ptr(dist), _ptr(labels), _ptr(mem_emb), _ptr(mem_dist), _ptr(mem_labels),
         _ptr(mem_state), _ptr(dembn), _ptr(loss), _ptr(coef), _ptr(mpick), _ptr(mcoef), _ptr(mine_info), batch, M, E, alpha, 1 if soft else 0,
         r=[region(embn), region(dist), region(labels), region(mem_dist)] + ring,
         w=[region(dembn), region(loss), region(coef), region(mpick), region(mcoef), region(mine_info)])
    emit(ops, "l2norm_bwd", lib.fn_l2norm_bwd, _ptr(emb), _ptr(dembn), _ptr(demb), batch, E, 1e-10,
         r=[region(emb), region(dembn)], w=[region(demb)])
    emit(ops, "xbm_enqueue", lib.fn_xbm_enqueue, _ptr(embn), _ptr(labels), _ptr(mem_emb), _ptr(mem_labels), _ptr(mem_state), batch, M, E,
         memory_start, r=[region(embn), region(labels), region(mem_state)], w=ring)
    return Head(ops, dict(embn=embn, dembn=dembn, dist=dist, coef=coef, labels=labels, mine_info=mine_info, mem_emb=mem_emb,
                          mem_labels=mem_labels, mem_state=mem_state, mem_dist=mem_dist, mpick=mpick, mcoef=mcoef),
                state=("mem_emb", "mem_labels", "mem_state"))


def _cls_desc(batch: int, L, dt: int):
    d = _lib.ConvDesc()
    d.N, d.H, d.W, d.Cin, d.OH, d.OW, d.Cout = batch, 1, 1, L.cin, 1, 1, L.cout
    d.KH = d.KW = d.stride = 1
    d.dtype, d.ld_x, d.ld_y, d.scale = dt, L.cin, L.cout, 1.0
    return d


def softmax_head(net: Network, emb: torch.Tensor, demb: torch.Tensor, loss: torch.Tensor, G: torch.Tensor, dt: int,
                 margin: Optional[Tuple[float, float, float]] = None) -> Head:
    """The classifier Dense(C), softmax cross-entropy, and the classifier's own weight and data gradients: its parameters are
    finished before the network's backward starts.  Plain: on the (un-normalised) embedding, with the bias.

    ``margin`` = (scale, arc, cos) makes it the large-margin cosine softmax: the classifier without
    bias on the L2-normalised embedding, cosines through the class rows' reciprocal norms, the margin in the label's column; the
    weight gradient gets the term of the row normalisation, the data gradient goes back through the embedding's normalisation.
    The bias stays in P, is not read and keeps a zero gradient."""
    lib, dev, (batch, E) = net.lib, net.device, emb.shape
    L = net.layers["classifier/logits"]
    Cp, Cr = L.cout, L.cout_real
    labels = torch.zeros(batch, dtype=torch.int32, device=dev)
    emb_lp = torch.zeros(batch, E, dtype=net.train_dtype, device=dev)
    logits = torch.zeros(batch, Cp, dtype=torch.float32, device=dev)
    dlogits = torch.zeros(batch, Cp, dtype=net.train_dtype, device=dev)
    tensors = dict(labels=labels, emb_lp=emb_lp, logits=logits, dlogits=dlogits)
    ops: List[Op] = []
    x, dx = emb, demb                       # what the classifier reads, where its data gradient goes
    if margin:
        assert L.w_off % 4 == 0 and E % 4 == 0, "the class rows are read with 16-byte loads"
        x = embn = torch.zeros(batch, E, dtype=torch.float32, device=dev)
        dx = dembn = torch.zeros(batch, E, dtype=torch.float32, device=dev)
        rnorm = torch.zeros(Cp, dtype=torch.float32, device=dev)
        margin_t = torch.zeros(Cp, dtype=torch.int64, device=dev)       # zeroed once: margin_wgrad_fix leaves it zeroed
        tensors.update(embn=embn, dembn=dembn, rnorm=rnorm, margin_t=margin_t)
        emit(ops, "l2norm_fwd", lib.fn_l2norm_fwd, _ptr(emb), _ptr(embn), batch, E, 1e-10, r=[region(emb)], w=[region(embn)])
    emit(ops, "cast_emb", lib.fn_cast_f32_to_lp, _ptr(x), _ptr(emb_lp), batch * E, dt, r=[region(x)], w=[region(emb_lp)])
    if margin:
        emit(ops, "margin_rnorm", lib.fn_margin_weight_rnorm, _ptr(net.P, L.w_off), Cr, E, 1e-10, _ptr(rnorm),
             r=[weight_region(net.P, L)], w=[region(rnorm)])
    d = _cls_desc(batch, L, dt)
    d.x, d.w, d.y, d.bias, d.out_f32 = _ptr(emb_lp), _ptr(net.W_train, L.w_off), _ptr(logits), None if margin else _ptr(net.P, L.bias_off), 1
    emit(ops, "conv_fwd:classifier", lib.fn_conv2d_fwd, C.byref(d), keep=(d,),
         r=[region(emb_lp), weight_region(net.W_train, L)] + ([] if margin else [bias_region(net.P, L)]), w=[region(logits)])
    if margin:
        emit(ops, "margin_softmax", lib.fn_margin_softmax_fwd_bwd, _ptr(logits), Cp, _ptr(rnorm), _ptr(labels),
             _ptr(loss), _ptr(dlogits), Cp, _ptr(margin_t), batch, Cr, *margin, 1.0 / batch, dt,
             r=[region(logits), region(rnorm), region(labels), region(margin_t)],
             w=[region(loss), region(dlogits), region(margin_t)])
    else:
        bias_acc = L.bias_off - net.bias_lo
        emit(ops, "softmax_xent", lib.fn_softmax_xent_fwd_bwd, _ptr(logits), Cp, _ptr(labels), _ptr(loss),
             _ptr(dlogits), Cp, _ptr(net.Gacc, bias_acc), batch, Cr, 1.0 / batch, dt,
             r=[region(logits), region(labels)],
             w=[region(loss), region(dlogits), region(net.Gacc, bias_acc, bias_acc + L.cout)])
    w = _cls_desc(batch, L, dt)
    w.x, w.y, w.dw = _ptr(emb_lp), _ptr(dlogits), _ptr(G, L.w_off)
    if margin:
        # This weight gradient has a consumer inside the step, so it stays where it is: group_wgrads moves the launches that carry
        # their descriptor in `keep` to the end of the segment, this one's descriptor is held by the head (Head.keep).
        # One split (the reduction runs over the batch only): a single ordered sum, no float atomics between workgroups.
        w.splits = 1
    emit(ops, "conv_wgrad:classifier", lib.fn_conv2d_wgrad, C.byref(w), keep=() if margin else (w,),
         r=[region(emb_lp), region(dlogits)], w=[weight_region(G, L)])
    if margin:
        emit(ops, "margin_wgrad_fix", lib.fn_margin_wgrad_fix, _ptr(G, L.w_off), _ptr(net.P, L.w_off), _ptr(rnorm),
             _ptr(margin_t), Cr, E,
             r=[weight_region(G, L), weight_region(net.P, L), region(rnorm), region(margin_t)],
             w=[weight_region(G, L), region(margin_t)])
    g = _cls_desc(batch, L, dt)
    g.y, g.w, g.dx, g.out_f32 = _ptr(dlogits), _ptr(net.Wt_train, L.w_off), _ptr(dx), 1
    emit(ops, "conv_dgrad:classifier", lib.fn_conv2d_dgrad, C.byref(g), keep=(g,),
         r=[region(dlogits), weight_region(net.Wt_train, L)], w=[region(dx)])
    if margin:
        emit(ops, "l2norm_bwd", lib.fn_l2norm_bwd, _ptr(emb), _ptr(dembn), _ptr(demb), batch, E, 1e-10,
             r=[region(emb), region(dembn)], w=[region(demb)])
    return Head(ops, tensors, keep=(w,) if margin else ())


def add_regularizers(head: Head, net: Network, emb: torch.Tensor, demb: torch.Tensor, center_factor: float, center_alfa: float,
                     prelogits_norm_factor: float, prelogits_norm_p: float, world: int, rank: int):
    """Center loss and prelogits norm on a softmax head: one launch after the classifier's data gradient
    adds their gradient into demb and reports the terms.  With center loss on it also writes this rank's (x, label) rows into
    center_rows [world, N, E+1]; the other ranks' slots arrive by an all-reduce (SUM) of the zeroed buffer -- an exact
    all-gather -- before center_update in the final segment, which therefore reads the gathered batch."""
    lib, dev, (N, E), labels = net.lib, net.device, emb.shape, head.tensors["labels"]
    n_classes = net.layers["classifier/logits"].cout_real
    reg_terms = head.tensors["reg_terms"] = torch.zeros(8, dtype=torch.float32, device=dev)    # zeroed once: the launch leaves its words zeroed
    reads, writes = [region(emb), region(labels), region(demb)], [region(demb), region(reg_terms)]
    centers = rows = None
    if center_factor > 0:
        centers = torch.zeros(n_classes, E, dtype=torch.float32, device=dev)     # tf.constant_initializer(0), not trainable
        center_rows = torch.zeros(world, N, E + 1, dtype=torch.float32, device=dev)
        head.tensors.update(centers=centers, center_rows=center_rows)
        head.state += ("centers",)
        rows = center_rows[rank]
        reads.append(region(centers))
        writes.append(region(center_rows, rank * N * (E + 1), (rank + 1) * N * (E + 1)))
        if world > 1:        # the other ranks' slots must be zero when the all-reduce sums them
            head.pre_ops.append(Op("zero_center_rows", torch_op(lambda: center_rows.zero_()), (), writes=(region(center_rows),)))
        emit(head.final_ops, "center_update", lib.fn_center_update, _ptr(center_rows), E + 1, world * N, E,
             _ptr(centers), centers.shape[0], center_alfa, r=[region(center_rows)], w=[region(centers)])
    emit(head.loss_ops, "center_loss", lib.fn_center_loss_fwd_bwd, _ptr(emb), _ptr(labels),
         None if centers is None else _ptr(centers), _ptr(demb), _ptr(reg_terms),
         None if rows is None else _ptr(rows), E + 1, N, E, n_classes, center_factor, prelogits_norm_factor,
         prelogits_norm_p, r=reads, w=writes)
