"""Training steps on the static-plan engine.

* ``Trainer(loss='softmax')`` is the reference's train step: ``Sequential([model, Dense(C)])`` +
  ``SparseCategoricalCrossentropy(from_logits=True)`` + ``Adam(epsilon=0.1)`` + Keras L2(5e-4)
  (apps/train_softmax.py:49-104; embedding NOT normalised in training, inception_resnet_v1.py:491).
* ``Trainer(loss='triplet')`` is the north-star path the reference lacks (build-defined
  from arXiv 1503.03832): forward(training=True) -> l2_normalize -> triplet loss over rows laid out
  (a0,p0,n0,a1,...).  ``TripletMiner`` does the online selection in a PxK pool on device.
* ``Trainer(loss='triplet', triplet_strategy='batch_hard' | 'batch_all', soft_margin=...)`` trains on the whole labelled P x K batch
  and mines inside it (arXiv 1703.07737 sec. 2): ``set_images(images, labels)``, no miner, no gather.
* ``Trainer(..., triplet_strategy='batch_hard', memory_size=M, memory_start=s)`` also mines over a cross-batch memory of the last M
  normalised rows of earlier steps (Wang et al., CVPR 2020); the labels are then dataset-wide identity ids.
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

The step lives here (segments, buckets, exchange, capture, checkpoint assembly); its parts live next door and are re-exported:
``heads`` (the loss heads), ``optimizers`` (the update rules, their state and checkpoint slots) and ``grouping`` (the
launch-list transformations: tile autotuning and grouped convolutions / weight gradients).
"""
from __future__ import annotations

import contextlib
import os
import warnings
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, heads, parallel
from .engine import Lowering, Network, _ptr
from .grouping import autotune_convs, group_convs, group_wgrads                                      # noqa: F401  (re-exported)
from .heads import check_loss_arguments
from .optimizers import (OPTIMIZERS, Optimizer, adam_beta_powers, check_moving_average_decay, check_optimizer,      # noqa: F401
                         moving_average_decay, optimizer_name)
from .schedule import Op, Schedule, StreamSet, emit, make_events, region, run_schedule, stats_region, torch_op


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
                 margin_arc: float = 0.0, margin_cos: float = 0.0, triplet_strategy: str = "mined", soft_margin: bool = False,
                 memory_size: int = 0, memory_start: int = 0):
        self.group_wgrad = group_wgrad
        self.optimizer = check_optimizer(optimizer)        # beta1, beta2 and epsilon are Adam's; the other rules' constants: OPTIMIZERS
        self.rule = OPTIMIZERS[self.optimizer]
        ema_decay = check_moving_average_decay(moving_average_decay)
        # force_segments: a single replica runs the data-parallel step structure (backward cut at the bucket boundaries, one graph
        # per segment, per-segment grouped weight gradients) with the all-reduce left out: what the segmentation alone costs
        # A process group given together with world_size == 1 still EXCHANGES: the bucket all-reduces run through that one-rank
        # communicator on the communication stream (identity on the data, the real backend calls and stream ordering) -- how
        # the RCCL path is exercised on a one-GPU box (bench.py --exchange-self, tests/test_gpu_dp.py).
        self.exchange = world_size > 1 or process_group is not None
        self.segmented = self.exchange or force_segments
        check_loss_arguments(net, batch, loss, center_factor, center_alfa, prelogits_norm_factor, prelogits_norm_p, margin_scale,
                             margin_arc, margin_cos, triplet_strategy, soft_margin, memory_size, memory_start)
        # "mined": rows (a,p,n,...) filled by a TripletMiner; "batch_hard" / "batch_all": mined inside the labelled batch (section 31)
        self.triplet_strategy, self.soft_margin = triplet_strategy, bool(soft_margin)
        self.batch_mined = loss == "triplet" and triplet_strategy != "mined"
        # a cross-batch memory of the last memory_size normalised rows, filled from step memory_start on (section 32); 0: none
        self.memory_size, self.memory_start = int(memory_size), int(memory_start)
        # NormFace / CosFace / ArcFace: settings, not state; margin_scale == 0 is the plain softmax head
        self.margin_scale, self.margin_arc, self.margin_cos = float(margin_scale), float(margin_arc), float(margin_cos)
        self.margin = margin_scale > 0
        self.center_factor, self.prelogits_norm_factor = float(center_factor), float(prelogits_norm_factor)
        self.regularized = center_factor > 0 or prelogits_norm_factor > 0
        self.net, self.N, self.loss_kind = net, batch, loss
        self.l2 = net.l2_weight if l2 is None else l2      # v1: L2_WEIGHT (Keras L2(5e-4)); v2: slim weight_decay / 2
        self.world, self.pg = world_size, process_group
        self.n_streams = n_streams
        dev, E, lib = net.device, net.E, net.lib
        self.lib = lib
        self.dt = _lib.dtype_code(net.train_dtype)
        if world_size > 1:
            # MirroredStrategy creates every replica from the SAME variables (apps/train_softmax_tf2_gpus.py:49-67): rank 0's
            # parameters and moving statistics win, whatever seed or file the other ranks were built from
            parallel.broadcast_parameters([net.P, net.S_mean, net.S_var], src=0, group=process_group)
            net.folded_valid = False
            net.refresh_packs()
        self.G = net.alloc_grads()       # + net.Gacc: fixed-point accumulators of the bias gradients (engine.Network.alloc_grads)
        # the update rule with what it keeps on the device: slots (under Adam M and V name its moments, the other rules leave them
        # None), hyper and the weights' moving average
        self.opt = Optimizer(net, self.G, self.optimizer, lr, beta1, beta2, epsilon, self.l2, 1.0 / world_size, ema_decay, self.dt)
        self.slots, self.hyper, self.shadow = self.opt.slots, self.opt.hyper, self.opt.shadow
        self.M, self.V = self.slots if self.optimizer == "ADAM" else (None, None)
        self.loss = torch.zeros(4, dtype=torch.float32, device=dev)     # [0] the loss; [1..3] the launch's flag + fixed-point accumulator
        # dropout (Inception-ResNet-v2) draws its masks from Keras' `iterations` word: forward and backward of a step read it
        # before the step's adam_tick, and graph replays see it advance; masks differ per data-parallel rank
        rank = 0
        if self.exchange:
            import torch.distributed as dist
            rank = dist.get_rank(process_group)
        self.rank = rank
        self.plan: Lowering = net.plan(batch, training=True, step_word=self.hyper.view(torch.int32)[4:5], rank=rank)
        self.demb = torch.zeros(batch, E, dtype=torch.float32, device=dev)
        self.emb = self.plan.embedding.buf.act.view(batch, E)
        if self.memory_size:
            head = heads.xbm_triplet_head(net, self.emb, self.demb, self.loss, alpha, self.soft_margin, self.memory_size, self.memory_start)
        elif self.batch_mined:
            head = heads.batch_triplet_head(net, self.emb, self.demb, self.loss, alpha, triplet_strategy, self.soft_margin)
        elif loss == "triplet":
            head = heads.triplet_head(net, self.emb, self.demb, self.loss, alpha)
        else:
            head = heads.softmax_head(net, self.emb, self.demb, self.loss, self.G, self.dt,
                                      (self.margin_scale, self.margin_arc, self.margin_cos) if self.margin else None)
            if self.regularized:
                heads.add_regularizers(head, net, self.emb, self.demb, self.center_factor, float(center_alfa), self.prelogits_norm_factor,
                                       float(prelogits_norm_p), world_size, rank)
        # the head's tensors are the trainer's attributes, bound here once: embn, dembn (triplet, margin); dist, coef, labels, mine_info
        # (batch-mined triplet); mem_emb, mem_labels, mem_state, mem_dist, mpick, mcoef (its cross-batch memory); labels, emb_lp, logits,
        # dlogits (softmax); rnorm, margin_t (margin); reg_terms, centers, center_rows (regularisers).  `head` itself stays: it
        # keeps what its launches point at alive
        self.head, self.centers = head, None
        for name, t in head.tensors.items():
            setattr(self, name, t)
        # every trainer-owned tensor a launch points at, by attribute name (slot<j>: the optimizer's slots)
        self.tensors: Dict[str, torch.Tensor] = dict(G=self.G, hyper=self.hyper, loss=self.loss, demb=self.demb, **head.tensors,
                                                     **{f"slot{j}": s for j, s in enumerate(self.slots)})
        if self.shadow is not None:
            self.tensors["shadow"] = self.shadow
        # what a step mutates and the next step reads: capture() snapshots it around its warm-up step
        self.state: List[torch.Tensor] = [net.P, net.S_mean, net.S_var, *self.slots, self.hyper, *(head.tensors[k] for k in head.state)]
        if self.shadow is not None:
            self.state.append(self.shadow)
        self.pre_ops: List[Op] = [
            Op("zero_grads", torch_op(lambda: (self.G.zero_(), net.Gacc.zero_())), (), writes=(region(self.G), region(net.Gacc))),
            Op("zero_bn_workspace", torch_op(lambda: (self.plan.ws.zero_(), self.plan.ws_b.zero_())), (),
               writes=(region(self.plan.ws), stats_region(self.plan.ws, 0, net.CB), region(self.plan.ws_b), stats_region(self.plan.ws_b, 0, net.CB))),
        ] + head.pre_ops
        self.loss_ops: List[Op] = head.loss_ops
        self.plan.build_backward(self.demb)
        self.opt_ops: List[Op] = self.opt.ops() + head.final_ops      # the final segment: under data parallelism it sees the gathered batch
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
        saved = [t.clone() for t in self.state]
        self.step_eager()           # warm-up: first-call attribute set-up, allocator
        torch.cuda.synchronize(net.device)
        for t, s in zip(self.state, saved):
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
        if labels is not None and self.batch_mined:
            # identity ids, any values: checked on the host, where it is cheap -- a batch in which no row has both a positive and
            # a negative would train on nothing without a word
            lab = np.asarray(torch.as_tensor(labels).cpu()).reshape(-1).astype(np.int64)
            if lab.size != self.N:
                raise ValueError(f"labels must hold one identity per batch row ({self.N}), got {lab.size}")
            if lab.min() < -2 ** 31 or lab.max() >= 2 ** 31:
                raise ValueError("labels must fit int32")
            _, inverse, counts = np.unique(lab, return_inverse=True, return_counts=True)
            # (with a cross-batch memory a row may find both in the memory: what the step had is in triplet_stats()["anchors"])
            if not self.memory_size and (len(counts) < 2 or not bool((counts[inverse] >= 2).any())):
                raise ValueError("no row of the batch has both a positive and a negative: the labels need at least two identities, one "
                                 "of them with two rows")
            self.labels.copy_(torch.from_numpy(lab.astype(np.int32)).to(self.net.device))
        elif labels is not None:
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
        out = {k: v.numpy() for k, v in self.net.keras_variables(self.averaged_moving_stats()).items()}
        out.update(self.opt.state_dict())
        out["epoch"] = np.asarray(int(epoch), dtype=np.int64)
        if self.centers is not None:
            out["centers:0"] = self.centers.cpu().numpy()      # the TF1 variable of facenet.py:208 (identical on every replica)
        out.update(self.opt.average_state_dict())
        if self.memory_size:                                   # this replica's ring: a resumed run mines against the same rows
            out["xbm/embeddings:0"] = self.mem_emb.cpu().numpy()
            out["xbm/labels:0"] = self.mem_labels.cpu().numpy()
            out["xbm/state:0"] = self.mem_state.cpu().numpy()
        return out

    def save_checkpoint(self, path, epoch: int = 0):
        sd = self.state_dict(epoch)          # collective when world > 1; rank 0 writes
        if self.world == 1 or int(os.environ.get("RANK", "0")) == 0:
            np.savez(path, **sd)

    def load_checkpoint(self, path) -> int:
        """Restore parameters, moving statistics and optimiser state; returns the stored epoch.  A checkpoint written under
        another optimizer restores everything but the optimizer, which starts fresh (Keras ``load_weights`` into a model
        compiled with another optimizer): initial slots, t = 0, this trainer's learning rate; a warning names both."""
        net = self.net
        with np.load(path, allow_pickle=False) as z:
            sd = {k: z[k] for k in z.files}
        optimizer_keys = tuple(r.keras + "/" for r in OPTIMIZERS.values())
        net.load_keras_params({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items() if not k.startswith(optimizer_keys + ("xbm/",)) and k != "epoch"})
        if self.centers is not None:
            if "centers:0" in sd:
                c = np.asarray(sd["centers:0"], dtype=np.float32)
                if c.shape != tuple(self.centers.shape):
                    raise ValueError(f"checkpoint centers:0 has shape {c.shape}, this trainer's centers are {tuple(self.centers.shape)}")
                self.centers.copy_(torch.from_numpy(c))
            else:
                self.centers.zero_()                            # a checkpoint from a run without center loss
        self.opt.load_state_dict(sd, path)
        if self.memory_size:
            self._load_memory(sd, path)
        return int(sd.get("epoch", 0))

    # ---- the cross-batch memory ---------------------------------------------------------------------
    def _require_memory(self):
        if not self.memory_size:
            raise RuntimeError("this Trainer keeps no cross-batch memory: build it with memory_size > 0")

    def reset_memory(self):
        """Empty the cross-batch memory; memory_start counts again from here."""
        self._require_memory()
        self.mem_state.zero_()

    def _load_memory(self, sd, path):
        keys = ("xbm/embeddings:0", "xbm/labels:0", "xbm/state:0")
        found = [np.asarray(sd[k]) for k in keys if k in sd]
        if len(found) == 3 and found[0].shape == tuple(self.mem_emb.shape) and found[1].shape == tuple(self.mem_labels.shape) \
                and found[2].shape == (4,):
            for t, a in zip((self.mem_emb, self.mem_labels, self.mem_state), found):
                t.copy_(torch.from_numpy(np.ascontiguousarray(a)).to(dtype=t.dtype))
            return
        why = "holds no cross-batch memory" if len(found) < 3 else f"holds a memory of {found[0].shape[0]} x {found[0].shape[-1]}"
        warnings.warn(f"checkpoint {path} {why}; this trainer's is {self.memory_size} x {self.net.E}: it starts empty")
        self.mem_state.zero_()

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
        """Keras' ``optimizer.iterations``: optimiser steps taken so far."""
        return self.opt.iterations

    @iterations.setter
    def iterations(self, t: int):
        self.opt.iterations = t

    def reset_optimizer(self, lr: Optional[float] = None):
        """The optimizer as freshly constructed: every slot at its initial value (Adam: zero moments; Adagrad: 0.1), t = 0."""
        self.opt.reset(lr)

    def set_learning_rate(self, lr: float):
        self.opt.set_learning_rate(lr)

    def loss_value(self) -> float:
        """The cross-entropy (softmax) or triplet loss of the last step, without the regularisers (see loss_terms)."""
        return float(self.loss[0].item())

    def triplet_stats(self) -> Dict[str, float]:
        """The last step's mining counts of a batch-mined triplet trainer (one small copy from the device): ``anchors`` (rows with a
        positive and a negative), ``terms``, ``active`` (hinge: terms > 0; soft margin: all of them) and ``active_fraction``.  With a cross-batch memory also
        ``memory_valid`` (the rows it held when the step mined) and ``memory_positives`` / ``memory_negatives`` (the anchors whose
        farthest positive / nearest negative was one of them)."""
        if not self.batch_mined:
            raise RuntimeError("triplet_stats() belongs to triplet_strategy 'batch_hard' / 'batch_all'")
        info = self.mine_info.cpu().tolist()
        anchors, terms, active = info[:3]
        out = {"anchors": anchors, "terms": terms, "active": active, "active_fraction": active / terms if terms else 0.0}
        if self.memory_size:      # the rows the memory held when the step mined, and the anchors whose pick came out of it
            out.update(memory_valid=info[6], memory_positives=info[4], memory_negatives=info[5])
        return out

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
