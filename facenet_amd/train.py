"""Training steps on the static-plan engine.

* ``Trainer(loss='softmax')`` is the reference's train step: ``Sequential([model, Dense(C)])`` +
  ``SparseCategoricalCrossentropy(from_logits=True)`` + ``Adam(epsilon=0.1)`` + Keras L2(5e-4)
  (apps/train_softmax.py:49-104; embedding NOT normalised in training, inception_resnet_v1.py:491).
* ``Trainer(loss='triplet')`` is the north-star path the reference lacks (build-defined
  from arXiv 1503.03832): forward(training=True) -> l2_normalize -> triplet loss over rows laid out
  (a0,p0,n0,a1,...).  ``TripletMiner`` does the online selection in a PxK pool on device.
* ``Trainer(loss='softmax', center_factor=..., prelogits_norm_factor=...)`` adds the reference's embedding regularisers
  (facenet/facenet.py:204-217 center loss, apps/configs/train_softmax.yaml:73-78 prelogits norm).
* ``Trainer(loss='softmax', margin_scale=64, margin_arc=0.5)`` replaces the plain softmax head by the large-margin cosine softmax
  (NormFace / CosFace / ArcFace) on the L2-normalised embedding and class rows.
* ``Trainer(..., moving_average_decay=0.9999)`` keeps TF1's ``ExponentialMovingAverage(decay, global_step)`` of the trainable
  variables (train.moving_average_decay, apps/configs/train_softmax.yaml:28), fused into the optimiser pass.
* ``Trainer(..., optimizer='RMSPROP')`` picks the update rule by the names of train.optimizer (apps/configs/train_softmax.yaml:25-26):
  ADAGRAD, ADADELTA, ADAM, RMSPROP, MOM, each the Keras optimizer the TF1 line's name maps to.
* Data parallelism restates ``tf.distribute.MirroredStrategy()`` (apps/train_softmax_tf2_gpus.py:49):
  one process per GPU, per-replica BatchNorm, gradients summed by RCCL all-reduce in backward-ordered
  buckets on a side stream (overlapped with the rest of backward), divided by the replica count
  inside the fused optimiser.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import json
import math
import os
import warnings
from typing import Callable, Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, parallel
from .config import Config
from .engine import BN_EPS, L2_WEIGHT, Lowering, Network, _pad8, _ptr, bias_region, weight_region
from .schedule import Op, Schedule, StreamSet, emit, levelize, make_events, region, run_schedule, stats_region, torch_op


class GraphRunner:
    """Capture launch schedules into HIP graphs (one per segment) and replay them.

    Segments exist so that collectives issued between them stay outside the captured graphs."""

    def __init__(self, device: torch.device):
        self.device = device
        self.graphs: List[torch.cuda.CUDAGraph] = []
        self.pool = None

    def capture(self, fn: Callable[[], None]) -> torch.cuda.CUDAGraph:
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, pool=self.pool):
            fn()
        if self.pool is None:
            self.pool = g.pool()
        self.graphs.append(g)
        return g


def _group_host(members: List[Op], nbytes: int):
    """Host tables of ONE grouped launch over ``members``: their descriptors, n opaque records of ``nbytes`` and the n + 1
    workgroup offsets, for the library's group-build call to fill."""
    n = len(members)
    return (_lib.ConvDesc * n)(*[m.keep[0] for m in members]), (C.c_uint8 * (nbytes * n))(), (C.c_int32 * (n + 1))()


def _group_upload(net: Network, members: List[Op], host_args, host_prefix):
    """Upload the filled tables once; the grouped launch reads and writes what its members did.
    -> (device records, device offsets, reads, writes)"""
    dev_args = torch.frombuffer(bytearray(host_args), dtype=torch.uint8).to(net.device)
    dev_prefix = torch.tensor(list(host_prefix), dtype=torch.int32, device=net.device)
    return dev_args, dev_prefix, tuple(r for m in members for r in m.reads), tuple(w for m in members for w in m.writes)


def group_wgrads(ops: List[Op], net: Network) -> List[Op]:
    """Weight gradients have no consumer before the optimiser (or the bucket all-reduce): pull every ``conv_wgrad`` launch
    out of ``ops`` and append ONE grouped launch per tile variant at the end (fn_conv2d_wgrad_grouped), planned once on the
    host.  Thousands of workgroups per launch instead of ~130 launches that each fill a fraction of the 256 CUs."""
    lib = net.lib
    singles = [op for op in ops if op.name.startswith("conv_wgrad:") and op.keep]
    if len(singles) < 2:
        return list(ops)
    out = [op for op in ops if not (op.name.startswith("conv_wgrad:") and op.keep)]
    groups = {}
    for op in singles:
        d = op.keep[0]
        v = lib.fn_conv2d_variant(C.byref(d), 2)
        norm = _lib.VARIANT_FLAG if d.nrm_stats and not _lib.variant_is_taps(v) else 0      # normalise-on-load members: their own groups
        groups.setdefault((v + norm, d.dtype), []).append(op)
    nbytes = lib.fn_conv2d_wgrad_arg_bytes()
    split_tables, split_keep, split_writes = [], [], []
    for (variant, dt), members in sorted(groups.items()):
        n = len(members)
        descs, host_args, host_prefix = _group_host(members, nbytes)
        ws_elems = C.c_int64(0)
        _lib.check(min(0, lib.fn_conv2d_wgrad_group_build(descs, n, variant, host_args, host_prefix, None, C.byref(ws_elems))),
                   "wgrad_group_build")                                                                     # sizing call
        # split layers write one fp32 slab per pixel split, summed in order by fn_conv2d_wgrad_reduce: no atomics, same bits every run
        ws = torch.empty(max(1, ws_elems.value), dtype=torch.float32, device=net.device)
        total = lib.fn_conv2d_wgrad_group_build(descs, n, variant, host_args, host_prefix, _ptr(ws), C.byref(ws_elems))
        _lib.check(min(0, total), "wgrad_group_build")
        dev_args, dev_prefix, reads, writes = _group_upload(net, members, host_args, host_prefix)
        kernel = "conv_wgrad_taps" if _lib.variant_is_taps(variant) else "conv_wgrad_grouped"
        out.append(Op(f"{kernel}:{_lib.variant_name(variant, wgrad=True)}", lib.fn_conv2d_wgrad_grouped,
                      (_ptr(dev_args), _ptr(dev_prefix), n, total, variant, dt), keep=(descs, dev_args, dev_prefix, members, ws),
                      reads=reads, writes=writes + (region(ws),)))
        if ws_elems.value > 0:
            split_tables.append(dev_args)
            split_keep.append(ws)
            split_writes.extend(writes)
    if split_tables:      # ONE ordered slab reduction for the split layers of every group (records of both kernels share a layout)
        table = torch.cat(split_tables)
        out.append(Op("conv_wgrad_reduce", lib.fn_conv2d_wgrad_reduce, (_ptr(table), table.numel() // nbytes), keep=(table, split_keep),
                      reads=tuple(region(w) for w in split_keep), writes=tuple(split_writes)))
    return out


TILE_CANDIDATES = tuple((bm, bn) for bm in (128, 64, 32) for bn in (128, 64, 32))


def autotune_convs(ops: Sequence[Op], net: Network, launches: int = 8, rounds: int = 2) -> Dict[str, int]:
    """Measure, don't guess: time every forward / data-gradient convolution of a plan with each tile variant (a burst of
    back-to-back launches between two HIP events, best of `rounds`) and write the winner into the descriptor
    (fn_conv_desc.tile_fwd / tile_dgrad).  The library heuristic stays the fallback (FACENET_AUTOTUNE=0) and the tie
    breaker: a candidate must beat it by 3 % to replace it.  Runs once per plan, before grouping and graph capture; what
    the launches write while being timed is overwritten or re-zeroed by the first real step."""
    if os.environ.get("FACENET_AUTOTUNE", "1") == "0":
        return {}
    lib, st = net.lib, net.stream()
    chosen: Dict[str, int] = {}
    # FACENET_TUNE_CACHE=<file>: reuse the tiles of an earlier run (same shapes) instead of timing again -- reproducible
    # plans, and profiles of a tuned run that do not contain the tuning bursts
    cache_path = os.environ.get("FACENET_TUNE_CACHE")
    cache: Dict[str, int] = {}
    if cache_path and os.path.exists(cache_path):
        with open(cache_path) as fh:
            cache = json.load(fh)
    dirty = False

    def burst(op):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(launches):
            rc = op.fn(*op.args, st)
            if rc:
                return float("inf")
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    for op in ops:
        kind = op.name.split(":")[0]
        if kind not in ("conv_fwd", "conv_dgrad") or not op.keep or not isinstance(op.keep[0], _lib.ConvDesc):
            continue
        d = op.keep[0]
        field = "tile_fwd" if kind == "conv_fwd" else "tile_dgrad"
        nout = d.Cout if kind == "conv_fwd" else d.Cin
        key = f"{op.name}|N{d.N}|{d.H}x{d.W}x{d.Cin}|dt{d.dtype}|nrm{int(bool(d.nrm_stats))}"
        if key in cache:
            setattr(d, field, int(cache[key]))
            chosen[op.name] = int(cache[key])
            continue
        setattr(d, field, 0)
        base_code = lib.fn_conv2d_variant(C.byref(d), 0 if kind == "conv_fwd" else 1)
        base = _lib.variant_tile(base_code)
        timings = {}
        if _lib.variant_is_halo(base_code):                       # the library's own choice is the halo-tile kernel: it competes as tile 0
            base = 0
            burst(op)
            timings[0] = min(burst(op) for _ in range(rounds))
        for bm, bn in TILE_CANDIDATES:
            if bn > 32 and bn // 2 >= nout:              # a tile twice as wide as the layer only multiplies zeros
                continue
            setattr(d, field, bm * 1000 + bn)
            burst(op)                                    # warm-up (code object, L2)
            timings[bm * 1000 + bn] = min(burst(op) for _ in range(rounds))
        best = min(timings, key=timings.get)
        if base in timings and timings[best] > 0.97 * timings[base]:
            best = base
        setattr(d, field, best)
        chosen[op.name] = best
        cache[key] = best
        dirty = True
    torch.cuda.synchronize()
    if cache_path and dirty:
        tmp = f"{cache_path}.{os.getpid()}.tmp"        # several ranks may share the file: replace it atomically
        with open(tmp, "w") as fh:
            json.dump(cache, fh, indent=0)
        os.replace(tmp, cache_path)
    return chosen


def group_convs(ops: List[Op], net: Network) -> List[Op]:
    """Order the launch list by dependency level (a valid topological order) and fuse same-level forward / data-gradient
    convolutions that share a tile variant into ONE grouped launch (fn_conv2d_grouped): sibling inception towers run as one
    kernel with 2-3x the workgroups instead of 2-3 under-occupied launches."""
    lib = net.lib
    level = levelize(ops)
    order = sorted(range(len(ops)), key=lambda i: (level[i], i))
    nbytes = lib.fn_conv2d_arg_bytes()
    buckets = {}
    for i in order:
        op = ops[i]
        kind = op.name.split(":")[0]
        if kind in ("conv_fwd", "conv_dgrad") and op.keep and isinstance(op.keep[0], _lib.ConvDesc) and not op.keep[0].dy2:
            d = op.keep[0]
            opi = 0 if kind == "conv_fwd" else 1
            if _lib.variant_is_halo(lib.fn_conv2d_variant(C.byref(d), opi)):
                continue                             # halo-tile kernel: a launch of its own
            plain = int(d.KH == 1 and d.KW == 1 and d.stride == 1 and d.pad_h == 0 and d.pad_w == 0)
            if opi == 0 and d.nrm_stats:
                plain |= 2                           # normalise-on-load members form their own groups
            buckets.setdefault((level[i], opi, lib.fn_conv2d_variant(C.byref(d), opi), plain, d.dtype), []).append(i)
    fused_at, skip = {}, set()
    for (lv, opi, variant, plain, dt), idxs in buckets.items():
        for c0 in range(0, len(idxs), 8):            # at most 8 layers per launch (linear scan in the kernel)
            chunk = idxs[c0:c0 + 8]
            if len(chunk) < 2:
                continue
            members, smem = [ops[i] for i in chunk], C.c_int32(0)
            descs, host_args, host_prefix = _group_host(members, nbytes)
            total = lib.fn_conv2d_group_build(descs, len(members), opi, variant, host_args, host_prefix, C.byref(smem))
            _lib.check(min(0, total), "conv_group_build")
            dev_args, dev_prefix, reads, writes = _group_upload(net, members, host_args, host_prefix)
            kname = "conv_fwd_grouped" if opi == 0 else "conv_dgrad_grouped"
            fused_at[chunk[0]] = Op(f"{kname}:{_lib.variant_name(variant)}:" + "+".join(m.name.split(":", 1)[1] for m in members),
                                   lib.fn_conv2d_grouped, (_ptr(dev_args), _ptr(dev_prefix), len(members), total, variant, plain, smem.value, dt),
                                   keep=(descs, dev_args, dev_prefix, members), reads=reads, writes=writes)
            skip.update(chunk[1:])
    out = []
    for i in order:
        if i in skip:
            continue
        out.append(fused_at.get(i, ops[i]))
    return out


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


def check_loss_arguments(net: Network, batch: int, loss: str, center_factor: float, center_alfa: float, prelogits_norm_factor: float,
                         prelogits_norm_p: float, margin_scale: float = 0.0, margin_arc: float = 0.0, margin_cos: float = 0.0):
    """What the Trainer refuses: an unknown loss, a batch or network that does not fit it, regulariser settings out of range
    (loss.center_factor / center_alfa / prelogits_norm_factor / prelogits_norm_p, train_softmax.yaml:73-78), margin settings out of
    range or without a scale (loss.margin_scale / margin_arc / margin_cos)."""
    if loss not in ("triplet", "softmax"):
        raise ValueError(f"unknown loss {loss!r}")
    if loss == "triplet" and batch % 3:
        raise ValueError("triplet batches are laid out (a,p,n,...): batch must be a multiple of 3")
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


def _streams_for(net: Network, n_streams: int) -> StreamSet:
    ss = getattr(net, "_stream_set", None)
    if ss is None or len(ss.side) < n_streams - 1:
        ss = StreamSet(net.device, n_streams)
        net._stream_set = ss
    return ss


class Trainer:
    def __init__(self, net: Network, batch: int, loss: str = "triplet", alpha: float = 0.2, lr: float = 0.05, beta1: float = 0.9,
                 beta2: float = 0.999, epsilon: float = 0.1, l2: Optional[float] = None, world_size: int = 1, process_group=None,
                 n_buckets: int = 6, n_streams: int = 1, group_wgrad: bool = True, force_segments: bool = False,
                 center_factor: float = 0.0, center_alfa: float = 0.95, prelogits_norm_factor: float = 0.0, prelogits_norm_p: float = 1.0,
                 moving_average_decay: Optional[float] = None, optimizer: str = "ADAM", margin_scale: float = 0.0,
                 margin_arc: float = 0.0, margin_cos: float = 0.0):
        self.group_wgrad = group_wgrad
        self.optimizer = check_optimizer(optimizer)        # beta1, beta2 and epsilon are Adam's; the other rules' constants: OPTIMIZERS
        self.rule = OPTIMIZERS[self.optimizer]
        self.ema_decay = check_moving_average_decay(moving_average_decay)
        # force_segments: a single replica runs the data-parallel step structure (backward cut at the bucket boundaries, one graph
        # per segment, per-segment grouped weight gradients) with the all-reduce left out: what the segmentation alone costs
        # A process group given together with world_size == 1 still EXCHANGES: the bucket all-reduces run through that one-rank
        # communicator on the communication stream (identity on the data, the real backend calls and stream ordering) -- how
        # the RCCL path is exercised on a one-GPU box (bench.py --exchange-self, tests/test_gpu_dp.py).
        self.exchange = world_size > 1 or process_group is not None
        self.segmented = self.exchange or force_segments
        check_loss_arguments(net, batch, loss, center_factor, center_alfa, prelogits_norm_factor, prelogits_norm_p, margin_scale,
                             margin_arc, margin_cos)
        # NormFace / CosFace / ArcFace: settings, not state; margin_scale == 0 is the plain softmax head
        self.margin_scale, self.margin_arc, self.margin_cos = float(margin_scale), float(margin_arc), float(margin_cos)
        self.margin = margin_scale > 0
        self.center_factor, self.center_alfa = float(center_factor), float(center_alfa)
        self.prelogits_norm_factor, self.prelogits_norm_p = float(prelogits_norm_factor), float(prelogits_norm_p)
        self.regularized = center_factor > 0 or prelogits_norm_factor > 0
        self.centers: Optional[torch.Tensor] = None
        self.net, self.N, self.loss_kind, self.alpha = net, batch, loss, alpha
        l2 = net.l2_weight if l2 is None else l2      # v1: L2_WEIGHT (Keras L2(5e-4)); v2: slim weight_decay / 2
        self.beta1, self.beta2, self.eps, self.l2 = beta1, beta2, epsilon, l2
        self.world, self.pg = world_size, process_group
        self.n_streams = n_streams
        dev, E, lib = net.device, net.E, net.lib
        self.lib = lib
        self.G = net.alloc_grads()       # + net.Gacc: fixed-point accumulators of the bias gradients (engine.Network.alloc_grads)
        # the optimizer's slot variables in the order of its OPTIMIZERS row, at their initial values; under Adam M and V name its
        # moments, the other rules leave them None
        self.slots: List[torch.Tensor] = [torch.full_like(self.G, init) for _, init in self.rule.slots]
        self.M, self.V = self.slots if self.optimizer == "ADAM" else (None, None)
        # hyper = {lr, beta1^t, beta2^t, grad_scale, t (int32 bits), 3 spare words}; lives on device so HIP-graph replays see
        # LR changes and advance Keras' step count themselves (fn_adam_tick: every rule; only Adam reads the beta powers)
        self.hyper = torch.tensor([lr, 1.0, 1.0, 1.0 / world_size, 0.0, 0.0, 0.0, 0.0], dtype=torch.float32, device=dev)
        self.loss = torch.zeros(4, dtype=torch.float32, device=dev)     # [0] the loss; [1..3] the launch's flag + fixed-point accumulator
        if world_size > 1:
            # MirroredStrategy creates every replica from the SAME variables (apps/train_softmax_tf2_gpus.py:49-67): rank 0's
            # parameters and moving statistics win, whatever seed or file the other ranks were built from
            parallel.broadcast_parameters([net.P, net.S_mean, net.S_var], src=0, group=process_group)
            net.folded_valid = False
            net.refresh_packs()
        # the moving average of every trainable variable (all of P; not the moving statistics, not the centers), initialised
        # from the weights every replica starts with; each replica applies the same update to the same reduced step: no exchange
        self.shadow: Optional[torch.Tensor] = None if self.ema_decay is None else net.P.clone()
        # dropout (Inception-ResNet-v2) draws its masks from Keras' `iterations` word: forward and backward of a step read it
        # before the step's adam_tick, and graph replays see it advance; masks differ per data-parallel rank
        rank = 0
        if self.exchange:
            import torch.distributed as dist
            rank = dist.get_rank(process_group)
        self.rank = rank
        self.plan: Lowering = net.plan(batch, training=True, step_word=self.hyper.view(torch.int32)[4:5], rank=rank)
        self.demb = torch.zeros(batch, E, dtype=torch.float32, device=dev)
        self.dt = _lib.dtype_code(net.train_dtype)
        emb = self.plan.embedding.buf.act
        self.emb = emb.view(batch, E)
        self.pre_ops: List[Op] = [
            Op("zero_grads", torch_op(lambda: (self.G.zero_(), net.Gacc.zero_())), (), writes=(region(self.G), region(net.Gacc))),
            Op("zero_bn_workspace", torch_op(lambda: (self.plan.ws.zero_(), self.plan.ws_b.zero_())), (),
               writes=(region(self.plan.ws), stats_region(self.plan.ws, 0, net.CB), region(self.plan.ws_b), stats_region(self.plan.ws_b, 0, net.CB))),
        ]
        self.loss_ops: List[Op] = []
        if loss == "triplet":
            self._build_triplet_loss(emb)
        else:
            if self.margin:
                self._build_margin_loss(emb)
            else:
                self._build_softmax_loss(emb)
            if self.regularized:
                self._build_regularizers()
        self.plan.build_backward(self.demb)
        self.opt_ops: List[Op] = []
        self._build_optimizer()
        n_buckets = int(os.environ.get("FACENET_DP_BUCKETS", n_buckets))      # tuning aid: gradient buckets of the data-parallel step
        self.buckets = self._make_buckets(n_buckets) if self.segmented else []
        self.comm_stream = torch.cuda.Stream(device=dev) if self.exchange else None
        self.streams = _streams_for(net, n_streams)
        self.tiles = autotune_convs(self.plan.fwd + self.loss_ops + self.plan.bwd, net)
        self._build_segments()
        self._graph = None
        self._exchange_events: Optional[dict] = None     # set by exchange_profile() around a step
        self._eval_plans: Dict[int, Tuple[Lowering, torch.Tensor]] = {}   # evaluate(): inference plan + output per batch size
        self._average_in_place = False      # inside averaged_weights(): P holds the moving average

    def _build_triplet_loss(self, emb: torch.Tensor):
        """l2_normalize -> triplet loss over rows (a0,p0,n0,a1,...) -> gradient wrt the un-normalised embedding (demb)."""
        net, lib, batch, E = self.net, self.lib, self.N, self.net.E
        self.embn = torch.zeros(batch, E, dtype=torch.float32, device=net.device)
        self.dembn = torch.zeros(batch, E, dtype=torch.float32, device=net.device)
        emit(self.loss_ops, "l2norm_fwd", lib.fn_l2norm_fwd, _ptr(emb), _ptr(self.embn), batch, E, 1e-10, r=[region(emb)], w=[region(self.embn)])
        emit(self.loss_ops, "triplet_loss", lib.fn_triplet_loss_fwd_bwd, _ptr(self.embn), _ptr(self.dembn), _ptr(self.loss),
             batch // 3, E, self.alpha, r=[region(self.embn)], w=[region(self.dembn), region(self.loss)])
        emit(self.loss_ops, "l2norm_bwd", lib.fn_l2norm_bwd, _ptr(emb), _ptr(self.dembn), _ptr(self.demb), batch, E, 1e-10,
             r=[region(emb), region(self.dembn)], w=[region(self.demb)])

    def _build_softmax_loss(self, emb: torch.Tensor):
        """The classifier Dense(C) on the (un-normalised) embedding, softmax cross-entropy, and the classifier's own weight and
        data gradients: its parameters are finished before the network's backward starts."""
        net, lib, batch, E, dev = self.net, self.lib, self.N, self.net.E, self.net.device
        L = net.layers["classifier/logits"]
        Cp, Cr = L.cout, L.cout_real
        self.labels = torch.zeros(batch, dtype=torch.int32, device=dev)
        self.emb_lp = torch.zeros(batch, E, dtype=net.train_dtype, device=dev)
        self.logits = torch.zeros(batch, Cp, dtype=torch.float32, device=dev)
        self.dlogits = torch.zeros(batch, Cp, dtype=net.train_dtype, device=dev)
        bias_acc = L.bias_off - net.bias_lo
        d = self._cls_desc(L)
        d.x, d.w, d.y, d.bias, d.out_f32 = _ptr(self.emb_lp), _ptr(net.W_train, L.w_off), _ptr(self.logits), _ptr(net.P, L.bias_off), 1
        emit(self.loss_ops, "cast_emb", lib.fn_cast_f32_to_lp, _ptr(emb), _ptr(self.emb_lp), batch * E, self.dt, r=[region(emb)], w=[region(self.emb_lp)])
        emit(self.loss_ops, "conv_fwd:classifier", lib.fn_conv2d_fwd, C.byref(d), keep=(d,),
             r=[region(self.emb_lp), weight_region(net.W_train, L), bias_region(net.P, L)], w=[region(self.logits)])
        emit(self.loss_ops, "softmax_xent", lib.fn_softmax_xent_fwd_bwd, _ptr(self.logits), Cp, _ptr(self.labels), _ptr(self.loss),
             _ptr(self.dlogits), Cp, _ptr(net.Gacc, bias_acc), batch, Cr, 1.0 / batch, self.dt,
             r=[region(self.logits), region(self.labels)],
             w=[region(self.loss), region(self.dlogits), region(net.Gacc, bias_acc, bias_acc + L.cout)])
        w = self._cls_desc(L)
        w.x, w.y, w.dw = _ptr(self.emb_lp), _ptr(self.dlogits), _ptr(self.G, L.w_off)
        emit(self.loss_ops, "conv_wgrad:classifier", lib.fn_conv2d_wgrad, C.byref(w), keep=(w,),
             r=[region(self.emb_lp), region(self.dlogits)], w=[weight_region(self.G, L)])
        g = self._cls_desc(L)
        g.y, g.w, g.dx, g.out_f32 = _ptr(self.dlogits), _ptr(net.Wt_train, L.w_off), _ptr(self.demb), 1
        emit(self.loss_ops, "conv_dgrad:classifier", lib.fn_conv2d_dgrad, C.byref(g), keep=(g,),
             r=[region(self.dlogits), weight_region(net.Wt_train, L)], w=[region(self.demb)])

    def _build_margin_loss(self, emb: torch.Tensor):
        """The large-margin cosine softmax head: the classifier without bias on the L2-normalised embedding,
        cosines through the class rows' reciprocal norms, the margin in the label's column; the weight gradient gets the term of
        the row normalisation, the data gradient goes back through the embedding's normalisation.  The bias stays in P, is not
        read and keeps a zero gradient."""
        net, lib, batch, E, dev = self.net, self.lib, self.N, self.net.E, self.net.device
        L = net.layers["classifier/logits"]
        Cp, Cr = L.cout, L.cout_real
        assert L.w_off % 4 == 0 and E % 4 == 0, "the class rows are read with 16-byte loads"
        self.labels = torch.zeros(batch, dtype=torch.int32, device=dev)
        self.embn = torch.zeros(batch, E, dtype=torch.float32, device=dev)
        self.dembn = torch.zeros(batch, E, dtype=torch.float32, device=dev)
        self.emb_lp = torch.zeros(batch, E, dtype=net.train_dtype, device=dev)
        self.logits = torch.zeros(batch, Cp, dtype=torch.float32, device=dev)
        self.dlogits = torch.zeros(batch, Cp, dtype=net.train_dtype, device=dev)
        self.rnorm = torch.zeros(Cp, dtype=torch.float32, device=dev)
        self.margin_t = torch.zeros(Cp, dtype=torch.int64, device=dev)       # zeroed once: margin_wgrad_fix leaves it zeroed
        ops = self.loss_ops
        emit(ops, "l2norm_fwd", lib.fn_l2norm_fwd, _ptr(emb), _ptr(self.embn), batch, E, 1e-10, r=[region(emb)], w=[region(self.embn)])
        emit(ops, "cast_emb", lib.fn_cast_f32_to_lp, _ptr(self.embn), _ptr(self.emb_lp), batch * E, self.dt,
             r=[region(self.embn)], w=[region(self.emb_lp)])
        emit(ops, "margin_rnorm", lib.fn_margin_weight_rnorm, _ptr(net.P, L.w_off), Cr, E, 1e-10, _ptr(self.rnorm),
             r=[weight_region(net.P, L)], w=[region(self.rnorm)])
        d = self._cls_desc(L)
        d.x, d.w, d.y, d.bias, d.out_f32 = _ptr(self.emb_lp), _ptr(net.W_train, L.w_off), _ptr(self.logits), None, 1
        emit(ops, "conv_fwd:classifier", lib.fn_conv2d_fwd, C.byref(d), keep=(d,),
             r=[region(self.emb_lp), weight_region(net.W_train, L)], w=[region(self.logits)])
        emit(ops, "margin_softmax", lib.fn_margin_softmax_fwd_bwd, _ptr(self.logits), Cp, _ptr(self.rnorm), _ptr(self.labels),
             _ptr(self.loss), _ptr(self.dlogits), Cp, _ptr(self.margin_t), batch, Cr, self.margin_scale, self.margin_arc,
             self.margin_cos, 1.0 / batch, self.dt,
             r=[region(self.logits), region(self.rnorm), region(self.labels), region(self.margin_t)],
             w=[region(self.loss), region(self.dlogits), region(self.margin_t)])
        # This weight gradient has a consumer inside the step, so it stays where it is: group_wgrads moves the launches that carry
        # their descriptor in `keep` to the end of the segment, this one keeps its descriptor on the trainer.  One split (the
        # reduction runs over the batch only): a single ordered sum, no float atomics between workgroups.
        w = self._margin_wgrad_desc = self._cls_desc(L)
        w.x, w.y, w.dw, w.splits = _ptr(self.emb_lp), _ptr(self.dlogits), _ptr(self.G, L.w_off), 1
        emit(ops, "conv_wgrad:classifier", lib.fn_conv2d_wgrad, C.byref(w),
             r=[region(self.emb_lp), region(self.dlogits)], w=[weight_region(self.G, L)])
        emit(ops, "margin_wgrad_fix", lib.fn_margin_wgrad_fix, _ptr(self.G, L.w_off), _ptr(net.P, L.w_off), _ptr(self.rnorm),
             _ptr(self.margin_t), Cr, E,
             r=[weight_region(self.G, L), weight_region(net.P, L), region(self.rnorm), region(self.margin_t)],
             w=[weight_region(self.G, L), region(self.margin_t)])
        g = self._cls_desc(L)
        g.y, g.w, g.dx, g.out_f32 = _ptr(self.dlogits), _ptr(net.Wt_train, L.w_off), _ptr(self.dembn), 1
        emit(ops, "conv_dgrad:classifier", lib.fn_conv2d_dgrad, C.byref(g), keep=(g,),
             r=[region(self.dlogits), weight_region(net.Wt_train, L)], w=[region(self.dembn)])
        emit(ops, "l2norm_bwd", lib.fn_l2norm_bwd, _ptr(emb), _ptr(self.dembn), _ptr(self.demb), batch, E, 1e-10,
             r=[region(emb), region(self.dembn)], w=[region(self.demb)])

    def _build_optimizer(self):
        """Step count and beta powers (fn_adam_tick) -> the update rule in one pass over P, with the moving average fused in when
        it is kept -> the transposed pack -> the centers (the final segment: under data parallelism it reads the gathered batch)."""
        net, lib, beta1, beta2, l2 = self.net, self.lib, self.beta1, self.beta2, self.l2
        emit(self.opt_ops, "adam_tick", lib.fn_adam_tick, _ptr(self.hyper), beta1, beta2, w=[region(self.hyper)])
        opt_writes = [region(net.P)] + [region(s) for s in self.slots] + [region(net.W_train)]
        rule, adam = self.rule, self.optimizer == "ADAM"
        # fn_adam_keras and fn_opt_keras are one pass of the same shape; fn_opt_keras takes its rule first, a one-slot rule no second slot
        fn, fn_ema = (lib.fn_adam_keras, lib.fn_adam_keras_ema) if adam else (lib.fn_opt_keras, lib.fn_opt_keras_ema)
        consts = (beta1, beta2, self.eps) if adam else (rule.rho, rule.momentum, rule.epsilon)
        opt_args = (() if adam else (rule.code,)) + (
            _ptr(net.P), _ptr(self.G), _ptr(self.slots[0]), _ptr(self.slots[1]) if len(self.slots) > 1 else None, _ptr(net.W_train),
            net.n_kernel, net.n_params, net.n_decay, _ptr(self.hyper), *consts, l2, self.dt)
        if self.shadow is None:
            emit(self.opt_ops, rule.op, fn, *opt_args, r=[region(self.G), region(self.hyper)], w=opt_writes)
        else:      # the same launch with the moving-average update fused in (one pass, same launch count)
            emit(self.opt_ops, rule.op + "_ema", fn_ema, *opt_args, _ptr(self.shadow), self.ema_decay,
                 r=[region(self.G), region(self.hyper)], w=opt_writes + [region(self.shadow)])
        emit(self.opt_ops, "pack_transpose", lib.fn_pack_transpose, _ptr(net.W_train), _ptr(net.Wt_train), _ptr(net.table),
             len(net.layers), net.max_layer_elems, self.dt, r=[region(net.W_train)], w=[region(net.Wt_train)])
        if self.centers is not None:
            emit(self.opt_ops, "center_update", lib.fn_center_update, _ptr(self.center_rows), net.E + 1, self.world * self.N, net.E,
                 _ptr(self.centers), self.centers.shape[0], self.center_alfa, r=[region(self.center_rows)], w=[region(self.centers)])

    def _build_regularizers(self):
        """Center loss and prelogits norm: one launch after the classifier's data gradient adds their
        gradient into demb and reports the terms.  With center loss on it also writes this rank's (x, label) rows into
        center_rows [world, N, E+1]; the other ranks' slots arrive by an all-reduce (SUM) of the zeroed buffer -- an exact
        all-gather -- before the final segment's center_update."""
        net, lib, N, E, dev, rank = self.net, self.net.lib, self.N, self.net.E, self.net.device, self.rank
        n_classes = net.layers["classifier/logits"].cout_real
        self.reg_terms = torch.zeros(8, dtype=torch.float32, device=dev)    # zeroed once: the launch leaves its words zeroed
        reads, writes = [region(self.emb), region(self.labels), region(self.demb)], [region(self.demb), region(self.reg_terms)]
        rows = None
        if self.center_factor > 0:
            self.centers = torch.zeros(n_classes, E, dtype=torch.float32, device=dev)     # tf.constant_initializer(0), not trainable
            self.center_rows = torch.zeros(self.world, N, E + 1, dtype=torch.float32, device=dev)
            rows = self.center_rows[rank]
            reads.append(region(self.centers))
            writes.append(region(self.center_rows, rank * N * (E + 1), (rank + 1) * N * (E + 1)))
            if self.world > 1:        # the other ranks' slots must be zero when the all-reduce sums them
                self.pre_ops.append(Op("zero_center_rows", torch_op(lambda: self.center_rows.zero_()), (), writes=(region(self.center_rows),)))
        emit(self.loss_ops, "center_loss", lib.fn_center_loss_fwd_bwd, _ptr(self.emb), _ptr(self.labels),
             None if self.centers is None else _ptr(self.centers), _ptr(self.demb), _ptr(self.reg_terms),
             None if rows is None else _ptr(rows), E + 1, N, E, n_classes, self.center_factor, self.prelogits_norm_factor,
             self.prelogits_norm_p, r=reads, w=writes)

    def _cls_desc(self, L):
        d = _lib.ConvDesc()
        d.N, d.H, d.W, d.Cin, d.OH, d.OW, d.Cout = self.N, 1, 1, L.cin, 1, 1, L.cout
        d.KH = d.KW = d.stride = 1
        d.dtype, d.ld_x, d.ld_y, d.scale = self.dt, L.cin, L.cout, 1.0
        return d

    # ---- data-parallel buckets -----------------------------------------------------------------
    def _make_buckets(self, n_buckets: int) -> List[Tuple[int, int, int]]:
        """[(bwd_op_index_after_which_ready, lo, hi)] over the flat gradient buffer, in backward order."""
        net = self.net
        layers = list(net.layers.values())
        done_at = {}
        for op_idx, li in self.plan.bwd_marks:
            done_at[li] = max(done_at.get(li, 0), op_idx)
        # the classifier (softmax) finishes inside the loss ops, i.e. before backward starts: done_at defaults to 0
        tail = (net.n_decay, net.n_params)
        buckets = parallel.make_buckets([L.w_off for L in layers], [L.numel for L in layers], done_at, net.n_kernel, tail,
                                        len(self.plan.bwd), n_buckets)
        parallel.check_buckets(buckets, net.n_kernel, tail)
        return buckets

    def _allreduce(self, lo: int, hi: int):
        parallel.allreduce_bucket(self.G, lo, hi, self.pg)

    def _build_segments(self):
        """world 1: one schedule for the whole step.  world > 1: the backward is cut where a gradient bucket becomes
        complete; every segment is its own multi-stream schedule (all streams joined at its end), and the bucket's
        all-reduce is issued on the communication stream while the next segment computes."""
        head = self.pre_ops + self.plan.fwd + self.loss_ops
        grp = (lambda ops: group_wgrads(group_convs(ops, self.net), self.net)) if self.group_wgrad else (lambda ops: list(ops))
        self.segments: List[Tuple[Optional[Schedule], Optional[Tuple[int, int]]]] = []
        if not self.segmented:
            chunks = int(os.environ.get("FACENET_WGRAD_CHUNKS", "0"))
            if chunks > 0 and self.group_wgrad:
                # experiment: the weight gradients leave the critical path -- the backward is cut into `chunks` pieces, each piece's
                # weight gradients become grouped launches pinned to a SIDE stream (they only feed the optimiser), everything else
                # stays on the main stream; the dgrad chain is latency-bound at a few % of the wave slots, the side stream fills them
                marks = [i for i, op in enumerate(self.plan.bwd) if op.name.startswith("conv_wgrad:")]
                cuts = [0] + [marks[len(marks) * k // chunks] for k in range(1, chunks)] + [len(self.plan.bwd)]
                ops: List[Op] = []
                for k in range(chunks):
                    ops += grp((head if k == 0 else []) + self.plan.bwd[cuts[k]:cuts[k + 1]])
                ops += self.opt_ops
                for op in ops:
                    op.stream_hint = 1 if op.name.startswith("conv_wgrad") else 0
                self.n_streams = max(2, self.n_streams)
                self.streams = _streams_for(self.net, self.n_streams)
                self.segments.append((Schedule(ops, self.n_streams), None))
                return
            self.segments.append((Schedule(grp(head + self.plan.bwd) + self.opt_ops, self.n_streams), None))
            return
        pos, first = 0, True
        for (ready, lo, hi) in self.buckets:
            a, b = pos, max(pos, ready)
            ops = grp((head if first else []) + self.plan.bwd[a:b])   # a bucket's weight gradients stay inside its segment
            self.segments.append((Schedule(ops, self.n_streams) if ops else None, (lo, hi)))
            pos, first = b, False
        assert pos == len(self.plan.bwd)
        self.segments.append((Schedule(self.opt_ops, 1), None))

    @property
    def step_ops(self) -> List[Op]:
        """The launches one step actually issues, in program order (after weight-gradient grouping)."""
        out: List[Op] = []
        for sched, _ in self.segments:
            if sched is not None:
                out.extend(sched.ops)
        return out

    # ---- one step ------------------------------------------------------------------------------
    def _zero(self):
        self.G.zero_()
        self.net.Gacc.zero_()
        self.plan.ws.zero_()
        self.plan.ws_b.zero_()

    def _run_segments(self, launch: Callable[[int], None]):
        self.net.folded_valid = False        # parameters and moving statistics are about to change
        if not self.segmented:
            launch(0)
            return
        if not self.exchange:                 # force_segments: the segment structure without the exchange
            for i, (sched, _) in enumerate(self.segments):
                if sched is not None:
                    launch(i)
            return
        cur = torch.cuda.current_stream(self.net.device)
        prof = self._exchange_events
        for i, (sched, rng) in enumerate(self.segments[:-1]):
            if sched is not None:
                launch(i)
            ev = torch.cuda.Event()
            ev.record(cur)
            self.comm_stream.wait_event(ev)
            with torch.cuda.stream(self.comm_stream):
                if i == 0 and self.centers is not None and self.world > 1:
                    # the head segment wrote this rank's center-loss rows: gather the global batch for center_update
                    import torch.distributed as dist
                    dist.all_reduce(self.center_rows, op=dist.ReduceOp.SUM, group=self.pg)
                if prof is not None:
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record(self.comm_stream)
                self._allreduce(*rng)
                if prof is not None:
                    b.record(self.comm_stream)
                    prof["buckets"].append((rng, a, b))
        if prof is not None:           # the compute stream has issued the whole backward: what is still exchanging now is exposed
            prof["bwd_end"] = torch.cuda.Event(enable_timing=True)
            prof["bwd_end"].record(cur)
        cur.wait_stream(self.comm_stream)
        launch(len(self.segments) - 1)

    def exchange_profile(self, steps: int = 3) -> dict:
        """Data-parallel runs: per-bucket all-reduce durations (HIP events on the communication stream) and the fraction of
        the exchange that ran while the compute stream was still inside backward (hidden) -- the rest delays the optimiser.
        Runs `steps` ordinary steps (they count as training steps) and reports their mean."""
        if not self.exchange:
            return {"buckets": [], "allreduce_ms": 0.0, "overlapped_frac": None}
        per_bucket, hidden, total = None, 0.0, 0.0
        for _ in range(steps):
            t0 = torch.cuda.Event(enable_timing=True)
            t0.record(torch.cuda.current_stream(self.net.device))
            self._exchange_events = {"buckets": []}
            try:
                self.step()
            finally:
                prof, self._exchange_events = self._exchange_events, None
            torch.cuda.synchronize(self.net.device)
            t_end = t0.elapsed_time(prof["bwd_end"])
            ms = []
            for (rng, a, b) in prof["buckets"]:
                ta, tb = t0.elapsed_time(a), t0.elapsed_time(b)
                ms.append(tb - ta)
                total += tb - ta
                hidden += max(0.0, min(tb, t_end) - min(ta, t_end))
            per_bucket = ms if per_bucket is None else [x + y for x, y in zip(per_bucket, ms)]
        return {"buckets": [{"elements": int(hi - lo), "mbytes": round(4e-6 * (hi - lo), 2), "allreduce_ms": round(m / steps, 4)}
                            for (_, lo, hi), m in zip(self.buckets, per_bucket)],
                "allreduce_ms": round(total / steps, 4), "overlapped_frac": round(hidden / total, 4) if total > 0 else None}

    def step_eager(self):
        """zero -> forward -> loss -> backward (+ bucketed all-reduce) -> optimizer; the loss stays on device."""
        self._run_segments(lambda i: run_schedule(self.segments[i][0], self.streams))

    def capture(self):
        """Capture every segment into a HIP graph (multi-stream edges become graph dependencies); with world_size > 1
        the all-reduces are issued between graph launches on the communication stream.

        Captured schedules span at most 2 streams.  Ending a capture whose fork / join pattern spans 3 or more streams
        segfaults inside hipStreamEndCapture under torch.cuda.graph on ROCm 7.0/7.2 (MI355X; 2 streams capture and replay
        correctly, and a single in-order stream replays fastest anyway: DESIGN.md section 5), so a wider trainer is refused
        here instead of being offered a way to crash a process that has initialised the GPU.  Eager replay
        (``step_eager``) keeps the requested width."""
        if self.n_streams > 2:
            raise ValueError(f"captured schedules span at most 2 streams (got n_streams={self.n_streams}); build the Trainer with "
                             f"n_streams <= 2 or replay eagerly (step_eager)")
        # The warm-up below is a full training step on whatever the image buffer holds.  Training state is snapshotted and
        # restored around it, so capture() followed by n steps equals n eager steps (the optimizer's t and slots, the moving
        # statistics and the parameters are untouched; the reference's fit() has no uncounted step either).
        net = self.net
        state = (net.P, net.S_mean, net.S_var, *self.slots, self.hyper) + tuple(t for t in (self.centers, self.shadow) if t is not None)
        saved = [t.clone() for t in state]
        self.step_eager()           # warm-up: first-call attribute set-up, allocator
        torch.cuda.synchronize(net.device)
        for t, s in zip(state, saved):
            t.copy_(s)
        net.folded_valid = False
        net.refresh_packs()
        torch.cuda.synchronize(net.device)
        runner = GraphRunner(self.net.device)
        graphs, keep = [], []
        for (sched, _) in self.segments:
            if sched is None:
                graphs.append(None)
                continue
            evs = make_events(sched)     # events owned by this capture only
            keep.append(evs)
            graphs.append(runner.capture(lambda sched=sched, evs=evs: run_schedule(sched, self.streams, evs)))
        self._graph = (runner, graphs, keep)

    def step(self):
        if self._graph is None:
            return self.step_eager()
        graphs = self._graph[1]
        self._run_segments(lambda i: graphs[i].replay())

    # ---- host conveniences -----------------------------------------------------------------------
    def set_images(self, images: torch.Tensor, labels: Optional[torch.Tensor] = None):
        self.plan.images.copy_(images.to(self.net.device, non_blocking=True))
        if labels is not None:
            if self.loss_kind != "softmax":
                raise ValueError("labels are only used by the softmax loss")
            labels = torch.as_tensor(labels)
            nc = self.net.layers["classifier/logits"].cout_real
            if labels.numel() != self.N or int(labels.min()) < 0 or int(labels.max()) >= nc:
                # TF's sparse softmax cross-entropy rejects out-of-range class indices; the kernel indexes logits[label]
                raise ValueError(f"labels must be {self.N} class indices in [0, {nc}), got range [{int(labels.min())}, {int(labels.max())}]")
            self.labels.copy_(labels.to(device=self.net.device, dtype=torch.int32))

    # ---- checkpoints (apps/train_softmax.py:68-78,105; SURVEY.md section 5: optimiser state) -----------------------------
    def averaged_moving_stats(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """BatchNorm moving statistics as MirroredStrategy reads them: every replica keeps its own (per-replica batch
        statistics), a read or save aggregates them with MEAN (apps/train_softmax_tf2_gpus.py:49).  Collective:
        every rank must call it."""
        mean, var = self.net.S_mean.clone(), self.net.S_var.clone()
        if self.world > 1:
            import torch.distributed as dist
            for t in (mean, var):
                dist.all_reduce(t, op=dist.ReduceOp.SUM, group=self.pg)
                t.mul_(1.0 / self.world)
        return mean, var

    def state_dict(self, epoch: int = 0) -> "Dict[str, np.ndarray]":
        """Model variables under their Keras names (replica-averaged moving statistics) + the Keras optimizer's slots
        ``<Optimizer>/<var>/<slot>`` (``Adam/<var>/m``, ``RMSprop/<var>/rms``, ...), ``<Optimizer>/iter``, its learning rate and
        the schedule position: everything ``fit`` needs to resume."""
        from . import keras_names
        net = self.net
        out = {k: v.numpy() for k, v in net.keras_variables(self.averaged_moving_stats()).items()}
        table = dict((i, k) for k, i in net.variable_table())
        prefix, slot_names = self.rule.keras, tuple(s for s, _ in self.rule.slots)
        for j, buf in enumerate(self.slots):
            for key, t in net.export_keras_grads(buf).items():
                out[keras_names.optimizer_slot_names(table[key], prefix, slot_names)[j]] = t.numpy()
        out[f"{prefix}/iter:0"] = np.asarray(self.iterations, dtype=np.int64)
        out[f"{prefix}/learning_rate:0"] = np.asarray(self.hyper[0].item(), dtype=np.float32)
        out["epoch"] = np.asarray(int(epoch), dtype=np.int64)
        if self.centers is not None:
            out["centers:0"] = self.centers.cpu().numpy()      # the TF1 variable of facenet.py:208 (identical on every replica)
        if self.shadow is not None:                            # TF1's shadow variables, next to the Adam slots
            for key, t in net.export_keras_grads(self.shadow).items():
                out[keras_names.moving_average_name(table[key])] = t.numpy()
        return out

    def save_checkpoint(self, path, epoch: int = 0):
        sd = self.state_dict(epoch)          # collective when world > 1; rank 0 writes
        if self.world == 1 or int(os.environ.get("RANK", "0")) == 0:
            np.savez(path, **sd)

    def load_checkpoint(self, path) -> int:
        """Restore parameters, moving statistics and optimiser state; returns the stored epoch.  A checkpoint written under
        another optimizer restores everything but the optimizer, which starts fresh (Keras ``load_weights`` into a model
        compiled with another optimizer): initial slots, t = 0, this trainer's learning rate; a warning names both."""
        from . import keras_names
        net = self.net
        with np.load(path, allow_pickle=False) as z:
            sd = {k: z[k] for k in z.files}
        optimizer_keys = tuple(r.keras + "/" for r in OPTIMIZERS.values())
        net.load_keras_params({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items() if not k.startswith(optimizer_keys) and k != "epoch"})
        if self.centers is not None:
            if "centers:0" in sd:
                c = np.asarray(sd["centers:0"], dtype=np.float32)
                if c.shape != tuple(self.centers.shape):
                    raise ValueError(f"checkpoint centers:0 has shape {c.shape}, this trainer's centers are {tuple(self.centers.shape)}")
                self.centers.copy_(torch.from_numpy(c))
            else:
                self.centers.zero_()                            # a checkpoint from a run without center loss
        prefix, slot_names = self.rule.keras, tuple(s for s, _ in self.rule.slots)
        saved_by = [name for name, r in OPTIMIZERS.items() if f"{r.keras}/iter:0" in sd]
        if f"{prefix}/iter:0" in sd:
            for slot, (buf, (_, init)) in enumerate(zip(self.slots, self.rule.slots)):
                tmp = {}
                for k, i in net.variable_table():
                    if i.endswith(("/moving_mean", "/moving_variance")):
                        continue
                    tmp[i] = torch.from_numpy(sd[keras_names.optimizer_slot_names(k, prefix, slot_names)[slot]])
                flat = net.flat_from_keras(tmp)
                if init != 0:      # the channel padding has no Keras value: it keeps the slot's initial value, as in a fresh trainer
                    real = net.flat_from_keras({i: torch.ones_like(t) for i, t in tmp.items()}) != 0
                    flat = torch.where(real, flat, torch.full_like(flat, init))
                buf.copy_(flat)
            self.hyper[0:1].fill_(float(sd[f"{prefix}/learning_rate:0"]))
            self.iterations = int(sd[f"{prefix}/iter:0"])
        elif saved_by:
            warnings.warn(f"checkpoint {path} holds {saved_by[0]} optimizer state but this trainer's optimizer is {self.optimizer}: "
                          f"the model variables are restored and the {self.optimizer} state starts fresh")
            self.reset_optimizer()
        if self.shadow is not None:
            trainable = [(k, i) for k, i in net.variable_table() if not i.endswith(("/moving_mean", "/moving_variance"))]
            if keras_names.moving_average_name(trainable[0][0]) in sd:
                self.shadow.copy_(net.flat_from_keras({i: torch.from_numpy(sd[keras_names.moving_average_name(k)]) for k, i in trainable}))
            else:                                               # a checkpoint of a run without the moving average
                self.reset_average()
        return int(sd.get("epoch", 0))

    # ---- the moving average of the weights ---------------------------------------------------------
    def _require_average(self):
        if self.shadow is None:
            raise RuntimeError("this Trainer keeps no moving average: build it with moving_average_decay in (0, 1)")

    def reset_average(self):
        """Restart the moving average from the current weights."""
        self._require_average()
        self.shadow.copy_(self.net.P)

    def averaged_variables(self) -> Dict[str, torch.Tensor]:
        """``keras_variables()`` with the moving average in place of every trainable variable and the replica-averaged moving
        statistics.  Collective under data parallelism: every rank must call it."""
        self._require_average()
        return self.net.keras_variables(self.averaged_moving_stats(), params=self.shadow)

    def save_averaged_weights(self, path):
        """The averaged model as an ``.npz`` with the keys and order of ``InceptionResnetV1.save_weights`` (readable by
        ``load_weights`` and ``FaceNet``).  Collective under data parallelism; rank 0 writes."""
        variables = self.averaged_variables()
        if self.rank == 0:
            np.savez(path, **{k: v.numpy() for k, v in variables.items()})

    @contextlib.contextmanager
    def averaged_weights(self):
        """Inside the block ``P`` holds the moving average: ``evaluate(..., averaged=True)`` calls swap and refold ONCE for the
        whole block instead of once per call (a validation pass over many batches).  ``P`` is restored bit for bit on exit and
        the fold is left to be redone; no training step may run inside the block."""
        self._require_average()
        if self._average_in_place:
            raise RuntimeError("averaged_weights() blocks do not nest")
        net = self.net
        saved = net.P.clone()
        net.P.copy_(self.shadow)
        net.folded_valid = False
        self._average_in_place = True
        try:
            yield self
        finally:
            self._average_in_place = False
            net.P.copy_(saved)
            net.folded_valid = False           # the fold holds the average: the next raw inference refolds

    def evaluate(self, images, averaged: bool = False) -> torch.Tensor:
        """L2-normalised inference embeddings [N, E] of uint8 NHWC images through the network's inference plan, from the raw
        weights or (``averaged``) from the moving average with this replica's moving statistics.  The inference plans read
        biases from ``P`` itself, so the average is swapped into ``P`` for the call and ``P`` is restored bit for bit after it."""
        net = self.net
        x = torch.as_tensor(images)
        S = net.image_size
        if x.dtype != torch.uint8 or x.dim() != 4 or tuple(x.shape[1:]) != (S, S, 3):
            raise ValueError(f"expected uint8 images [N,{S},{S},3], got {x.dtype} {tuple(x.shape)}")
        if averaged:
            self._require_average()
        elif self._average_in_place:
            raise RuntimeError("inside averaged_weights() the raw weights are swapped out: evaluate with averaged=True")
        n = x.shape[0]
        if n > 256:      # the per-plan batch limit of inference (InceptionResnetV1.MAX_PLAN_BATCH)
            return torch.cat([self.evaluate(x[i:i + 256], averaged) for i in range(0, n, 256)])
        st = net.stream()
        if n not in self._eval_plans:
            self._eval_plans[n] = (net.plan(n, training=False), torch.empty(n, net.E, dtype=torch.float32, device=net.device))
        plan, out = self._eval_plans[n]
        plan.images.copy_(x.to(net.device))
        saved = None
        try:
            if averaged and not self._average_in_place:
                saved = net.P.clone()
                net.P.copy_(self.shadow)
                net.folded_valid = False
            net.refresh_folded(st, force=False)
            Lowering.run_ops(plan.fwd, st)
            _lib.check(self.lib.fn_l2norm_fwd(_ptr(plan.embedding.buf.act), _ptr(out), n, net.E, 1e-10, st), "l2norm")
            return out.clone()
        finally:
            if saved is not None:
                net.P.copy_(saved)
                net.folded_valid = False       # the fold holds the average: the next raw inference refolds

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

    def reset_optimizer(self, lr: Optional[float] = None):
        """The optimizer as freshly constructed: every slot at its initial value (Adam: zero moments; Adagrad: 0.1), t = 0."""
        for buf, (_, init) in zip(self.slots, self.rule.slots):
            buf.fill_(init)
        self.iterations = 0
        if lr is not None:
            self.set_learning_rate(lr)

    def set_learning_rate(self, lr: float):
        self.hyper[0:1].fill_(float(lr))     # device write: visible to the next graph replay

    def loss_value(self) -> float:
        """The cross-entropy (softmax) or triplet loss of the last step, without the regularisers (see loss_terms)."""
        return float(self.loss[0].item())

    def loss_terms(self) -> Dict[str, Optional[float]]:
        """The last step's terms under the names the reference logged: ``xent``, ``center_loss``, ``prelogits_norm`` and their
        weighted sum ``loss`` (xent + center_factor * center_loss + prelogits_norm_factor * prelogits_norm).  A term that is
        switched off is None; the prelogits norm is reported whenever a regulariser is on, even at factor 0."""
        xent = self.loss_value()
        center = norm = None
        if self.regularized:
            t = self.reg_terms[:2].cpu().tolist()
            norm = float(t[1])
            if self.centers is not None:
                center = float(t[0])
        total = xent
        if center is not None:
            total += self.center_factor * center
        if self.prelogits_norm_factor > 0:
            total += self.prelogits_norm_factor * norm
        return {"xent": xent, "center_loss": center, "prelogits_norm": norm, "loss": total}


def check_gather_bytes(bytes_per_image: int) -> int:
    """fn_gather_images copies whole 16-byte vectors; say so when the miner is built, not in the middle of a step."""
    if bytes_per_image <= 0 or bytes_per_image % 16 != 0:
        raise ValueError(f"{bytes_per_image} bytes per image is not a multiple of 16: the triplet batch is gathered as 16-byte vectors "
                         "(an odd image size such as 299 x 299 x 3 is not supported)")
    return bytes_per_image


class TripletMiner:
    """Embeds a PxK pool with the inference path, selects triplets on device and assembles the train batch."""

    def __init__(self, net: Network, pool_size: int, labels: Sequence[int], nrof_triplets: int, alpha: float = 0.2, seed: int = 0,
                 semi_hard: bool = False, n_streams: int = 1, group: bool = True):
        self.group = group
        self.net, self.n, self.T, self.alpha, self.seed, self.semi_hard = net, pool_size, nrof_triplets, alpha, seed, semi_hard
        dev = net.device
        self.n_streams = n_streams
        lab = np.asarray(list(labels))
        if lab.shape != (pool_size,):
            raise ValueError(f"labels must have one entry per pool image ({pool_size}), got {lab.shape}")
        _, counts = np.unique(lab, return_counts=True)
        pairs = int((counts * (counts - 1) // 2).sum())
        # every selected triplet needs its own anchor-positive pair and a negative of another identity: a pool that cannot
        # supply them would leave triplet slots unwritten (the gather would reuse stale indices)
        if len(counts) < 2 or pairs < nrof_triplets:
            raise ValueError(f"the pool holds {len(counts)} identities and {pairs} anchor-positive pairs; {nrof_triplets} triplets need "
                             f">= 2 identities and >= {nrof_triplets} pairs")
        if pairs > 1 << 15:
            raise ValueError(f"{pairs} anchor-positive pairs exceed the 32768 the on-device ranking handles; use more identities with fewer images each")
        self.plan = net.plan(pool_size, training=False)
        E = net.E
        self.emb = self.plan.embedding.buf.act.view(pool_size, E)
        self.embn = torch.zeros(pool_size, E, dtype=torch.float32, device=dev)
        self.dist = torch.zeros(pool_size, pool_size, dtype=torch.float32, device=dev)
        self.labels = torch.as_tensor(list(labels), dtype=torch.int32).to(dev)
        self.triplets = torch.zeros(nrof_triplets, 3, dtype=torch.int32, device=dev)
        qmax = pool_size * (pool_size - 1) // 2
        self.info = torch.zeros(8 + 5 * qmax, dtype=torch.int32, device=dev)
        self.ops: List[Op] = []
        self.sched: Optional[Schedule] = None
        self.streams = _streams_for(net, n_streams)

    def build(self, train_images: torch.Tensor):
        """train_images: the uint8 [3T,H,W,3] input buffer of the training plan (filled by the gather)."""
        net, lib, n, E = self.net, self.net.lib, self.n, self.net.E
        o = self.ops
        bytes_per = check_gather_bytes(train_images[0].numel() * train_images.element_size())
        o.append(Op("fold_bn", lambda st: (net.refresh_folded(st), 0)[1], (),
                    reads=(region(net.P), region(net.S_mean), region(net.S_var)), writes=(region(net.W_infer), region(net.fold_bias))))
        net.refresh_folded(net.stream())          # the inference pack must exist before launches are timed
        self.tiles = autotune_convs(self.plan.fwd, net)
        o.extend(self.plan.fwd)
        emit(o, "l2norm_fwd", lib.fn_l2norm_fwd, _ptr(self.emb), _ptr(self.embn), n, E, 1e-10, r=[region(self.emb)], w=[region(self.embn)])
        emit(o, "pairwise_sqdist", lib.fn_pairwise_sqdist, _ptr(self.embn), _ptr(self.embn), _ptr(self.dist), None, n, n, E, 2,
             r=[region(self.embn)], w=[region(self.dist)])
        emit(o, "select_triplets", lib.fn_select_triplets, _ptr(self.dist), _ptr(self.labels), n, self.alpha, self.T, self.seed,
             1 if self.semi_hard else 0, _ptr(self.triplets), _ptr(self.info),
             r=[region(self.dist), region(self.labels)], w=[region(self.triplets), region(self.info)])
        emit(o, "gather_images", lib.fn_gather_images, _ptr(self.plan.images), _ptr(self.triplets), _ptr(train_images), 3 * self.T, bytes_per,
             r=[region(self.plan.images), region(self.triplets)], w=[region(train_images)])
        self.ops = group_convs(o, net) if self.group else o
        self.sched = Schedule(self.ops, self.n_streams)

    def run(self, events=None):
        run_schedule(self.sched, self.streams, events)
