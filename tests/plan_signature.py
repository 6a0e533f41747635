"""Host-only launch-list signature of a lowered plan (test helper).

A network is built with ``allocate=False`` and given CPU tensors and a stub library, so ``Network.plan`` and
``Lowering.build_backward`` run without a GPU.  Every launch becomes (name, library function, arguments), with each pointer
argument rewritten as (tensor role, byte offset) and every ConvDesc spelled out field by field.  Two revisions of the engine
that lower a network to the same signature issue the same kernels with the same arguments.

``regions=True`` appends every launch's read and write regions (what ``levelize``, ``group_convs`` and ``Schedule`` order the
launches by), ``trainer_signature`` does the same for a whole ``Trainer`` step, and ``CASES`` names the plans and trainers that
``tests/golden/plan_signatures.json`` pins (``python -m tests.plan_signature FILE`` records them)."""
import contextlib
import ctypes as C
import hashlib
import json
import os
import sys

import torch


class _StubLib:
    def __getattr__(self, name):
        def fn(*args):
            raise RuntimeError(f"stub {name} called")
        fn.__name__ = name
        return fn


def _stub_network(net):
    dev = torch.device("cpu")
    net.device = dev
    net.lib = _StubLib()
    net.P = torch.zeros(net.n_params)
    net.S_mean, net.S_var = torch.zeros(net.CB), torch.ones(net.CB)
    net.W_train = torch.zeros(net.n_kernel, dtype=net.train_dtype)
    net.Wt_train = torch.zeros(net.n_kernel, dtype=net.train_dtype)
    net.W_infer = torch.zeros(net.n_kernel, dtype=net.infer_dtype)
    net.fold_bias = torch.zeros(net.CB)
    net.table = torch.zeros(len(net.layers), 8, dtype=torch.int32)
    net.G = None
    net.alloc_grads()
    return net


def _tensors(net, plan):
    out = {}
    for k in ("P", "S_mean", "S_var", "W_train", "Wt_train", "W_infer", "fold_bias", "G", "Gacc", "table"):
        out["net." + k] = getattr(net, k)
    for k, v in vars(plan).items():
        if isinstance(v, torch.Tensor):
            out["plan." + k] = v
    for name, b in plan.bufs.items():
        for part in ("act", "raw", "grad"):
            t = getattr(b, part)
            if t is not None:
                out[f"buf.{name}.{part}"] = t
    for i, r in enumerate(plan.recs):
        for k, v in r.extra.items():
            if isinstance(v, torch.Tensor):
                out[f"rec{i}.{k}"] = v
    for k, v in getattr(plan, "_dup", {}).items():
        out["dup." + k] = v
    return out


def _trainer_tensors(tr):
    return {"tr." + k: t for k, t in tr.tensors.items()}


def _spans(tensors):
    return sorted(((n, t.data_ptr(), t.data_ptr() + t.numel() * t.element_size()) for n, t in tensors.items() if t.numel() > 0),
                  key=lambda s: (s[1], s[0]))


def _canon(v, spans, keep_ints=False):
    """``keep_ints``: a large integer that lies in no tensor and below every user-space heap address (a parameter count, a byte
    count) keeps its value instead of becoming an unknown pointer."""
    if isinstance(v, C.Structure):
        return [(f, _canon(getattr(v, f), spans, keep_ints)) for f, _ in v._fields_]
    if isinstance(v, C.Array):
        return [_canon(e, spans, keep_ints) for e in v]
    if isinstance(v, C.c_void_p):
        v = v.value
    if isinstance(v, C._Pointer) or type(v).__name__ == "CArgObject":
        v = C.cast(v._obj if hasattr(v, "_obj") else v, C.c_void_p).value
    if isinstance(v, int) and v > (1 << 20):
        # a pointer inside a tensor names that tensor; one past a tensor's end names it only when no tensor starts there (two
        # allocations that happen to be adjacent must not make the role depend on the allocator)
        for name, lo, hi in spans:
            if lo <= v < hi:
                return ("ptr", name, v - lo)
        for name, lo, hi in spans:
            if v == hi:
                return ("ptr", name, v - lo)
        if keep_ints and v < (1 << 32):
            return v
        return ("ptr", "?")
    if isinstance(v, float):
        return round(v, 9)
    return v


def _region_bases(tensors):
    """Region base -> (role, 0 | 1): a tensor's data_ptr(), or data_ptr() + 1 for the statistics view of plan.ws / plan.ws_b."""
    bases = {}
    for name, t in sorted(tensors.items()):
        if t.numel() > 0:
            bases.setdefault(t.data_ptr(), (name, 0))
    for name in ("plan.ws", "plan.ws_b"):
        if name in tensors:
            bases[tensors[name].data_ptr() + 1] = (name, 1)
    return bases


def _canon_ops(ops, tensors, regions):
    spans, bases = _spans(tensors), _region_bases(tensors)
    out = []
    for op in ops:
        args = []
        for a in op.args:
            if type(a).__name__ == "CArgObject":       # C.byref(desc)
                a = a._obj
            args.append(_canon(a, spans, keep_ints=regions))
        fn = "torch_op" if getattr(op.fn, "_torch_op", False) else getattr(op.fn, "__name__", "torch_op")
        row = [op.name, fn, args]
        if regions:
            row += [[list(bases.get(b, ("?", 0))) + [lo, hi] for (b, lo, hi) in regs] for regs in (op.reads, op.writes)]
        out.append(row)
    return out


def signature(net, N, training, loss="triplet", regions=False):
    """[(op name, function name, canonical arguments)] of the forward (and, for training plans, backward) launch list;
    ``regions``: each entry also carries its canonical read and write regions [(role, 0 | 1, lo, hi)]."""
    _stub_network(net)
    plan = net.plan(N, training=training, loss=loss if training else None)
    if training:
        plan.build_backward(torch.zeros(N, net.E))
    return _canon_ops(plan.fwd + (plan.bwd if training else []), _tensors(net, plan), regions)


@contextlib.contextmanager
def _environ(env):
    saved = {k: os.environ.get(k) for k in env}
    for k, v in env.items():            # None: unset
        os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    try:
        yield
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def trainer_signature(net, batch, **kw):
    """The whole step of ``Trainer(net, batch, group_wgrad=False, **kw)`` on the stubbed network, before grouping:
    {"launches": pre_ops + plan.fwd + loss_ops + plan.bwd + opt_ops in canonical form with regions, "buckets": tr.buckets}."""
    from facenet_amd.train import Trainer
    _stub_network(net)
    with _environ({"FACENET_AUTOTUNE": "0"}):
        tr = Trainer(net, batch, group_wgrad=False, **kw)
    tensors = dict(_tensors(net, tr.plan), **_trainer_tensors(tr))
    ops = tr.pre_ops + tr.plan.fwd + tr.loss_ops + tr.plan.bwd + tr.opt_ops
    return {"launches": _canon_ops(ops, tensors, True), "buckets": [list(b) for b in tr.buckets]}


# ---- the pinned cases: key -> (environment, builder) ----------------------------------------------------------------------------
def _v1(N, training, E=128, loss="triplet", **kw):
    from facenet_amd.engine import Network
    return lambda: signature(Network(E, allocate=False, device="cpu", **kw), N, training, loss=loss, regions=True)


def _v2(N, training, **cfg):
    from facenet_amd.engine_v2 import NetworkV2
    return lambda: signature(NetworkV2(128, allocate=False, device="cpu", config=dict(repeat=[2, 2, 2], **cfg)), N, training, regions=True)


def _block(kind, H, W, Cc, N, training, **kw):
    from facenet_amd.engine import BlockNetwork
    return lambda: signature(BlockNetwork(kind, H, W, Cc, allocate=False, device="cpu", **kw), N, training, regions=True)


def _block_v2(stages, HW, Cc, N, keep=1.0):
    from facenet_amd.engine_v2 import BlockNetworkV2
    from tests.irv2_oracle import BLOCK_E, BLOCK_SEED
    return lambda: signature(BlockNetworkV2(stages, HW, HW, Cc, embedding_size=BLOCK_E, config={"keep_probability": keep}, seed=BLOCK_SEED,
                                            allocate=False, device="cpu"), N, True, regions=True)


# the lone stages and chains of Inception-ResNet-v2: key -> case of tests/irv2_oracle.BLOCK_CASES, the table tests/test_gpu_irv2_blocks.py
# runs (stages, input map, channels, N, keep), so the recorded plan is the plan that test lowers
V2_BLOCK_KEYS = {
    "v2_mixed_5a_train_4": "mixed_5a", "v2_block35_x2_train_4": "block35_x2", "v2_mixed_6a_train_8": "mixed_6a",
    "v2_block17_x2_train_8": "block17_x2", "v2_mixed_7a_train_48": "mixed_7a", "v2_block8_x2_train_48": "block8_x2",
    "v2_block8_last_train_48": "block8_last", "v2_chain_35_6a_17_train_8": "chain_35_6a_17", "v2_chain_17_7a_8_train_48": "chain_17_7a_8",
    "v2_tail_train_48_dropout": "tail_keep_half", "v2_tail_train_48_keep_all": "tail_keep_1", "v2_block35_299_train_2": "g299_block35",
    "v2_tail_299_train_48_dropout": "g299_tail_keep_half",
}


def _v2_block_plans():
    from tests.irv2_oracle import BLOCK_CASES
    plans = {key: BLOCK_CASES[case] for key, case in V2_BLOCK_KEYS.items()}
    assert all(key.endswith((f"_train_{spec[3]}", f"_train_{spec[3]}_dropout", f"_train_{spec[3]}_keep_all")) for key, spec in plans.items())
    return plans


V2_BLOCK_PLANS = _v2_block_plans()


def _trainer(loss="triplet", **kw):
    from facenet_amd.engine import Network
    classes = 10 if loss == "softmax" else None
    return lambda: trainer_signature(Network(128, allocate=False, device="cpu", nrof_classes=classes), 6, loss=loss, **kw)


OPTION_VARS = ("FACENET_NORM_ON_LOAD", "FACENET_LAZY_BN_MAXHW", "FACENET_LAZY_BN_KMAX", "FACENET_MERGE_SIBLINGS", "FACENET_FUSE_RESIDUAL_BWD",
               "FACENET_FUSE_BLOCKS", "FACENET_FUSE_BLOCKS_MIN_BATCH", "FACENET_WARM_AHEAD", "FACENET_DP_BUCKETS", "FACENET_WGRAD_CHUNKS")
TRAIN_OPTIONS = {"FACENET_NORM_ON_LOAD": "1", "FACENET_LAZY_BN_MAXHW": "17", "FACENET_MERGE_SIBLINGS": "0", "FACENET_FUSE_RESIDUAL_BWD": "0"}
REGULARIZED = dict(center_factor=0.01, center_alfa=0.9, prelogits_norm_factor=5e-4, moving_average_decay=0.9999)

CASES = {
    "v1_train_6": ({}, _v1(6, True)),
    "v1_train_6_norm_on_load": ({"FACENET_NORM_ON_LOAD": "1"}, _v1(6, True)),
    "v1_train_6_lazy_bn_17": ({"FACENET_LAZY_BN_MAXHW": "17"}, _v1(6, True)),
    "v1_train_6_lazy_bn_17_kmax_300": ({"FACENET_LAZY_BN_MAXHW": "17", "FACENET_LAZY_BN_KMAX": "300"}, _v1(6, True)),
    "v1_train_6_no_merge_no_fuse": ({"FACENET_MERGE_SIBLINGS": "0", "FACENET_FUSE_RESIDUAL_BWD": "0"}, _v1(6, True)),
    "v1_train_6_softmax": ({}, _v1(6, True, loss="softmax", nrof_classes=10)),
    "v1_infer_32": ({}, _v1(32, False)),
    "v1_infer_32_no_fuse_blocks": ({"FACENET_FUSE_BLOCKS": "0"}, _v1(32, False)),
    "v1_infer_32_no_warm_ahead": ({"FACENET_WARM_AHEAD": "0"}, _v1(32, False)),
    "v1_infer_32_min_batch_33": ({"FACENET_FUSE_BLOCKS_MIN_BATCH": "33"}, _v1(32, False)),
    "v1_infer_16_min_batch_16": ({"FACENET_FUSE_BLOCKS_MIN_BATCH": "16"}, _v1(16, False)),
    "v1_infer_32_training_options": (TRAIN_OPTIONS, _v1(32, False)),
    "v2_train_6_dropout": ({}, _v2(6, True)),
    "v2_train_6_keep_all": ({}, _v2(6, True, keep_probability=1.0)),
    "v2_infer_6": ({}, _v2(6, False)),
    "block35_train_6": ({}, _block("block35", 17, 17, 256, 6, True, repeat=2)),
    "block17_train_6": ({}, _block("block17", 8, 8, 896, 6, True, scale=0.1, repeat=2)),
    "block8_train_6": ({}, _block("block8", 3, 3, 1792, 6, True, scale=0.2, repeat=2)),
    "reduction_a_train_6": ({}, _block("reduction_a", 17, 17, 256, 6, True)),
    "reduction_b_train_6": ({}, _block("reduction_b", 8, 8, 896, 6, True)),
    "block35_infer_32": ({}, _block("block35", 17, 17, 256, 32, False, repeat=2)),
    "block17_infer_32": ({}, _block("block17", 8, 8, 896, 32, False, scale=0.1, repeat=2)),
    **{key: ({}, _block_v2(*spec)) for key, spec in V2_BLOCK_PLANS.items()},
    "trainer_triplet": ({}, _trainer()),
    "trainer_softmax": ({}, _trainer("softmax")),
    "trainer_triplet_force_segments": ({}, _trainer(force_segments=True)),
    **{f"trainer_softmax_regularized_{name.lower()}": ({}, _trainer("softmax", optimizer=name, **REGULARIZED))
       for name in ("ADAGRAD", "ADADELTA", "ADAM", "RMSPROP", "MOM")},
    "trainer_softmax_margin_arcface": ({}, _trainer("softmax", margin_scale=64, margin_arc=0.5)),
    "trainer_softmax_margin_regularized_rmsprop": ({}, _trainer("softmax", margin_scale=30, margin_arc=0.3, margin_cos=0.1, optimizer="RMSPROP",
                                                                **REGULARIZED)),
    "trainer_softmax_regularized_force_segments": ({}, _trainer("softmax", force_segments=True, **REGULARIZED)),
}


def lowered(key):
    """The canonical signature of one case, lowered under the case's environment."""
    env, build = CASES[key]
    with _environ(dict(dict.fromkeys(OPTION_VARS), **env)):      # every option the case does not set is at its default
        return build()


def digest(key, sig=None):
    """{"ops": launches, "sha256": of the canonical JSON} of one case (``sig``: its signature, when already lowered)."""
    sig = lowered(key) if sig is None else sig
    n = len(sig["launches"] if isinstance(sig, dict) else sig)
    return {"ops": n, "sha256": hashlib.sha256(json.dumps(sig, sort_keys=True).encode()).hexdigest()}


if __name__ == "__main__":      # python -m tests.plan_signature OUT.json: record every case with the engine of this checkout
    with open(sys.argv[1], "w") as fh:
        json.dump({k: digest(k) for k in CASES}, fh, indent=1, sort_keys=True)
        fh.write("\n")
