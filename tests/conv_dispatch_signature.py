"""Host-only signature of the convolution dispatch in libfacenet_hip.so (test helper).

Which kernel instantiation a descriptor runs, and the argument records the grouped launches are planned from, are decided by
pure host code in the library: ``fn_conv2d_variant``, ``fn_conv2d_group_build`` and the sizing call (``ws = NULL``) of
``fn_conv2d_wgrad_group_build`` need the built library but no device.  The descriptors come from the stub lowering of
``tests/plan_signature.py`` plus a hand-written list of edge cases; every non-null pointer field is rewritten to a fake address
that depends only on the field's position, so the records the library fills are the same bytes in every process.  Two
revisions of ``csrc/`` with the same signature send every descriptor to the same kernel with the same arguments.

``python -m tests.conv_dispatch_signature FILE`` records ``tests/golden/conv_dispatch_signatures.json``."""
import ctypes as C
import hashlib
import json
import sys

import torch

from facenet_amd import _lib
from tests.plan_signature import OPTION_VARS, V2_BLOCK_PLANS, _environ, _stub_network
from tests.util import conv_desc

POINTER_FIELDS = [f for f, t in _lib.ConvDesc._fields_ if t is C.c_void_p]
HALO = _lib.VARIANT_HALO
TILES = [bm * 1000 + bn for bm in (128, 64, 32) for bn in (128, 64, 32)]


def fake_pointers(d):
    """Every non-null pointer becomes 256 MiB + 1 MiB * (its index among the pointer fields); null stays null."""
    for i, f in enumerate(POINTER_FIELDS):
        if getattr(d, f):
            setattr(d, f, (256 + i) << 20)
    return d


def _copy(d):
    e = _lib.ConvDesc()
    C.memmove(C.byref(e), C.byref(d), C.sizeof(d))
    return e


def _sha(buf):
    return hashlib.sha256(bytes(buf)).hexdigest()


def _error(lib):
    return lib.fn_last_error().decode("utf-8", "replace")


def conv_group(lib, descs, op, variant):
    """fn_conv2d_group_build over ``descs``: the negative status and its message, or total, smem, prefix and one hash per record."""
    n, nbytes = len(descs), lib.fn_conv2d_arg_bytes()
    arr, args, prefix, smem = (_lib.ConvDesc * n)(*descs), (C.c_uint8 * (nbytes * n))(), (C.c_int32 * (n + 1))(), C.c_int32(0)
    total = lib.fn_conv2d_group_build(arr, n, op, variant, args, prefix, C.byref(smem))
    if total < 0:
        return {"status": total, "error": _error(lib)}
    return {"total": total, "smem": smem.value, "prefix": list(prefix), "records": [_sha(args[i * nbytes:(i + 1) * nbytes]) for i in range(n)]}


def wgrad_group(lib, descs, variant):
    """The sizing call of fn_conv2d_wgrad_group_build over ``descs``."""
    n, nbytes = len(descs), lib.fn_conv2d_wgrad_arg_bytes()
    arr, args, prefix, ws_elems = (_lib.ConvDesc * n)(*descs), (C.c_uint8 * (nbytes * n))(), (C.c_int32 * (n + 1))(), C.c_int64(0)
    total = lib.fn_conv2d_wgrad_group_build(arr, n, variant, args, prefix, None, C.byref(ws_elems))
    if total < 0:
        return {"status": total, "error": _error(lib)}
    return {"total": total, "ws_elems": ws_elems.value, "prefix": list(prefix), "records": [_sha(args[i * nbytes:(i + 1) * nbytes]) for i in range(n)]}


def descriptor_signature(lib, d):
    """What the library decides for one descriptor, as every operation: the variant, and for variants that can be grouped the
    one-member group built from it."""
    out = {}
    for op in (0, 1, 2):
        v = lib.fn_conv2d_variant(C.byref(d), op)
        out[f"variant{op}"] = v
        if v < 0 or (op < 2 and _lib.variant_is_halo(v)):
            continue
        if op == 2 and d.nrm_stats and not _lib.variant_is_taps(v):
            v += _lib.VARIANT_FLAG                                      # as train.group_wgrads asks for it
        out[f"group{op}"] = conv_group(lib, [d], op, v) if op < 2 else wgrad_group(lib, [d], v)
    return out


# ---- descriptors of whole plans ---------------------------------------------------------------------------------------------------
def _lower(net, N, training):
    _stub_network(net)
    plan = net.plan(N, training=training, loss="triplet" if training else None)
    if training:
        plan.build_backward(torch.zeros(N, net.E))
    return plan


def _v1(N, training):
    from facenet_amd.engine import Network
    return lambda: _lower(Network(128, allocate=False, device="cpu"), N, training)


def _v2(N, training):
    from facenet_amd.engine_v2 import NetworkV2
    return lambda: _lower(NetworkV2(128, allocate=False, device="cpu"), N, training)


def _block(kind, HW, Cc, N, training, **kw):
    from facenet_amd.engine import BlockNetwork
    return lambda: _lower(BlockNetwork(kind, HW, HW, Cc, allocate=False, device="cpu", **kw), N, training)


def _block_v2(stages, HW, Cc, N, keep=1.0):
    from facenet_amd.engine_v2 import BlockNetworkV2
    from tests.irv2_oracle import BLOCK_E, BLOCK_SEED
    return lambda: _lower(BlockNetworkV2(stages, HW, HW, Cc, embedding_size=BLOCK_E, config={"keep_probability": keep}, seed=BLOCK_SEED,
                                         allocate=False, device="cpu"), N, True)


PLANS = {
    "v1_train_90": ({}, _v1(90, True)),
    "v1_infer_180_no_fuse_blocks": ({"FACENET_FUSE_BLOCKS": "0"}, _v1(180, False)),
    "v1_infer_8_no_fuse_blocks": ({"FACENET_FUSE_BLOCKS": "0"}, _v1(8, False)),
    "v2_train_16": ({}, _v2(16, True)),
    # the single-block plans of tests/plan_signature.CASES
    "block35_train_6": ({}, _block("block35", 17, 256, 6, True, repeat=2)),
    "block17_train_6": ({}, _block("block17", 8, 896, 6, True, scale=0.1, repeat=2)),
    "block8_train_6": ({}, _block("block8", 3, 1792, 6, True, scale=0.2, repeat=2)),
    "reduction_a_train_6": ({}, _block("reduction_a", 17, 256, 6, True)),
    "reduction_b_train_6": ({}, _block("reduction_b", 8, 896, 6, True)),
    "block35_infer_32_no_fuse_blocks": ({"FACENET_FUSE_BLOCKS": "0"}, _block("block35", 17, 256, 32, False, repeat=2)),      # (fused: no convolution launch)
    "block17_infer_32_no_fuse_blocks": ({"FACENET_FUSE_BLOCKS": "0"}, _block("block17", 8, 896, 32, False, scale=0.1, repeat=2)),
    # the lone stages and chains of Inception-ResNet-v2 of tests/plan_signature.V2_BLOCK_PLANS
    **{key: ({}, _block_v2(*spec)) for key, spec in V2_BLOCK_PLANS.items()},
    "v1_train_6_norm_on_load": ({"FACENET_NORM_ON_LOAD": "1"}, _v1(6, True)),
    "v1_train_6_lazy_bn_17": ({"FACENET_LAZY_BN_MAXHW": "17"}, _v1(6, True)),
    "v1_train_6_no_merge_siblings": ({"FACENET_MERGE_SIBLINGS": "0"}, _v1(6, True)),
    "v1_train_6_no_fuse_residual_bwd": ({"FACENET_FUSE_RESIDUAL_BWD": "0"}, _v1(6, True)),
}


def conv_ops(ops):
    return [op for op in ops if op.name.split(":")[0] in ("conv_fwd", "conv_dgrad", "conv_wgrad") and op.keep and isinstance(op.keep[0], _lib.ConvDesc)]


def lowered(key):
    """The plan of PLANS[key] under its environment, the pointers of every convolution descriptor already faked (in place: the
    launch arguments refer to the same objects)."""
    env, build = PLANS[key]
    with _environ(dict(dict.fromkeys(OPTION_VARS), **env)):
        plan = build()
    for op in conv_ops(plan.fwd + plan.bwd):
        fake_pointers(op.keep[0])
    return plan


def plan_signature(lib, plan):
    """{"convs": n, "sha256": of [(launch name, descriptor signature)]} over the convolution launches of a plan."""
    rows = [[op.name, descriptor_signature(lib, op.keep[0])] for op in conv_ops(plan.fwd + plan.bwd)]
    return {"convs": len(rows), "sha256": hashlib.sha256(json.dumps(rows, sort_keys=True).encode()).hexdigest()}


# ---- the groups a Trainer forms ---------------------------------------------------------------------------------------------------
class _HostNet:
    """What train.group_convs / group_wgrads need of a network, with the tables 'uploaded' to host memory."""
    device = torch.device("cpu")

    def __init__(self, lib):
        self.lib = lib


def plan_groups(lib, plan):
    """The multi-member launches train.group_convs and train.group_wgrads form from the forward and the backward list, each
    built again here from its members: {launch name: group signature}."""
    from facenet_amd.train import group_convs, group_wgrads
    net, out = _HostNet(lib), {}
    for part, ops in (("fwd", plan.fwd), ("bwd", plan.bwd)):
        for g in group_wgrads(group_convs(list(ops), net), net):
            kind = g.name.split(":")[0]
            if kind in ("conv_fwd_grouped", "conv_dgrad_grouped"):
                variant, plain, dt = g.args[4], g.args[5], g.args[7]
                sig = dict(conv_group(lib, list(g.keep[0]), 0 if kind == "conv_fwd_grouped" else 1, variant), variant=variant, plain=plain, dtype=dt)
                assert sig["total"] == g.args[3] and sig["smem"] == g.args[6]
            elif kind in ("conv_wgrad_grouped", "conv_wgrad_taps"):
                variant, dt = g.args[4], g.args[5]
                sig = dict(wgrad_group(lib, list(g.keep[0]), variant), variant=variant, dtype=dt, members=[m.name for m in g.keep[3]])
                assert sig["total"] == g.args[3]
            else:
                continue
            assert f"{part}:{g.name}" not in out
            out[f"{part}:{g.name}"] = sig
    return out


def rejected_groups(lib, plan):
    """Members that must not share a launch: the status and the message of the build call."""
    fwd = [op.keep[0] for op in conv_ops(plan.fwd) if not _lib.variant_is_halo(lib.fn_conv2d_variant(C.byref(op.keep[0]), 0))]
    dgrad = [op.keep[0] for op in conv_ops(plan.bwd) if op.name.startswith("conv_dgrad:")]
    is_plain = lambda d: d.KH == 1 and d.KW == 1 and d.stride == 1 and d.pad_h == 0 and d.pad_w == 0
    variant = lambda d, op=0: lib.fn_conv2d_variant(C.byref(d), op)
    plain = next(d for d in fwd if is_plain(d))
    general = next(d for d in fwd if not is_plain(d) and variant(d) == variant(plain))
    other_tile = next(d for d in fwd if is_plain(d) and variant(d) != variant(plain))
    f16 = _copy(plain)
    f16.dtype = _lib.FN_F16
    sibling = next(d for d in dgrad if d.dy2)
    single = next(d for d in dgrad if not d.dy2 and is_plain(d) and variant(d, 1) == variant(sibling, 1))
    wg = [op.keep[0] for op in conv_ops(plan.bwd) if op.name.startswith("conv_wgrad:") and not _lib.variant_is_taps(variant(op.keep[0], 2))]
    wg_other = next(d for d in wg if variant(d, 2) != variant(wg[0], 2))
    wg_f16 = _copy(wg[0])
    wg_f16.dtype = _lib.FN_F16
    return {
        "fwd_plain_with_general": conv_group(lib, [plain, general], 0, variant(plain)),
        "fwd_two_tiles": conv_group(lib, [plain, other_tile], 0, variant(plain)),
        "fwd_two_dtypes": conv_group(lib, [plain, f16], 0, variant(plain)),
        "dgrad_sibling_sources": conv_group(lib, [single, sibling], 1, variant(single, 1)),
        "wgrad_two_tiles": wgrad_group(lib, [wg[0], wg_other], variant(wg[0], 2)),
        "wgrad_two_dtypes": wgrad_group(lib, [wg[0], wg_f16], variant(wg[0], 2)),
        "wgrad_norm_flag_without_norm": wgrad_group(lib, [wg[0]], variant(wg[0], 2) + _lib.VARIANT_FLAG),
    }


# ---- hand-written edge descriptors ------------------------------------------------------------------------------------------------
def _desc(case, dt=_lib.FN_BF16, **fields):
    d = conv_desc(*case, dt)
    d.x = d.w = d.y = d.dx = d.dw = 1            # any non-null value: fake_pointers() gives them their addresses
    for k, v in fields.items():
        setattr(d, k, v)
    return fake_pointers(d)


def edge_descriptors():
    """{name: descriptor}.  Cases are (N, H, W, Cin, Cout, kh, kw, stride, pad_h, pad_w) as in tests/test_gpu_conv.py."""
    out = {}
    halo_cases = [(2, 37, 37, 80, 192, 3, 3, 1, 0, 0), (2, 40, 33, 32, 64, 3, 3, 1, 1, 1), (1, 45, 39, 32, 32, 3, 3, 1, 0, 0),
                  (2, 35, 35, 192, 80, 3, 3, 1, 0, 0)]
    for i, case in enumerate(halo_cases):            # the heuristic, an explicit request, an explicit implicit-GEMM tile
        for tile in (0, HALO, 64064):
            out[f"halo{i}_tile{tile}"] = _desc(case, tile_fwd=tile, tile_dgrad=tile)
    near = {"small_map_17": (2, 17, 17, 32, 32, 3, 3, 1, 1, 1), "map_31_out_29": (2, 31, 31, 32, 32, 3, 3, 1, 0, 0),
            "map_32_out_30": (2, 32, 32, 32, 32, 3, 3, 1, 0, 0), "channels_72": (2, 40, 40, 72, 72, 3, 3, 1, 1, 1),
            "channels_64": (2, 40, 40, 64, 64, 3, 3, 1, 1, 1), "stride_2": (2, 41, 41, 32, 32, 3, 3, 2, 0, 0),
            "1x1": (2, 17, 17, 64, 64, 1, 1, 1, 0, 0), "5x5": (2, 40, 40, 32, 32, 5, 5, 1, 2, 2), "1x3": (2, 40, 40, 32, 32, 1, 3, 1, 0, 1)}
    for name, case in near.items():
        for tile in (0, HALO):
            out[f"near_halo_{name}_tile{tile}"] = _desc(case, tile_fwd=tile, tile_dgrad=tile)
    out["near_halo_f16"] = _desc(halo_cases[2], _lib.FN_F16)
    for name, case in {"dgrad_s2_odd_17": (2, 17, 17, 192, 256, 3, 3, 2, 0, 0), "dgrad_s2_odd_19": (2, 19, 19, 8, 32, 3, 3, 2, 0, 0),
                       "dgrad_s2_odd_rect": (3, 21, 15, 64, 96, 3, 3, 2, 0, 0), "dgrad_s2_1x1": (2, 17, 17, 64, 64, 1, 1, 2, 0, 0)}.items():
        out[name] = _desc(case)
    b17 = (3, 8, 8, 128, 128, 1, 7, 1, 0, 3)          # block17 1x7: not a layer of the halo-tile kernel
    for tile in TILES + [HALO, 48048, -1]:
        out[f"tile_fwd_{tile}"] = _desc(b17, tile_fwd=tile)
        out[f"tile_dgrad_{tile}"] = _desc(b17, tile_dgrad=tile)
    for name, case in {"deep_k_few_tiles": (2, 8, 8, 1792, 32, 1, 1, 1, 0, 0), "deep_k_64_rows": (6, 8, 8, 128, 128, 7, 1, 1, 3, 0),
                       "dense": (7, 1, 1, 1792, 128, 1, 1, 1, 0, 0), "ragged_cout": (3, 9, 9, 64, 80, 1, 1, 1, 0, 0)}.items():
        out[name] = _desc(case)
    null = conv_desc(2, 17, 17, 256, 32, 1, 1, 1, 0, 0, _lib.FN_BF16)
    out["null_pointers"] = null
    out["null_pointers_deep_k"] = conv_desc(2, 8, 8, 1792, 32, 1, 1, 1, 0, 0, _lib.FN_BF16)
    out["null_pointers_bad_ld"] = _desc((2, 17, 17, 256, 32, 1, 1, 1, 0, 0), ld_y=20)
    out["bad_dtype"] = _desc((2, 17, 17, 256, 32, 1, 1, 1, 0, 0), dtype=7)
    norm = dict(nrm_stats=1, nrm_beta=1, nrm_count=128, nrm_eps=1e-3, nrm_sq_off=1792, nrm_replicas=2, nrm_rep_stride=4096)
    out["k512"] = _desc((2, 8, 8, 512, 32, 1, 1, 1, 0, 0))                               # splits K in the launch ...
    out["norm_on_load_k512"] = _desc((2, 8, 8, 512, 32, 1, 1, 1, 0, 0), **norm)          # ... unless it normalises on load
    out["norm_on_load_too_deep"] = _desc((2, 8, 8, 1792, 32, 1, 1, 1, 0, 0), **norm)     # rejected (Cin > 512), the variant still answers
    out["norm_on_load_3x3"] = _desc((2, 17, 17, 32, 32, 3, 3, 1, 1, 1), **norm)
    out["norm_on_load_without_beta"] = _desc((2, 17, 17, 32, 32, 3, 3, 1, 1, 1), **dict(norm, nrm_beta=None))
    out["sibling_sources"] = _desc((2, 17, 17, 256, 32, 1, 1, 1, 0, 0), dy2=1, w2=1, Cout2=32, ld_y2=32, dy3=1, w3=1, Cout3=48, ld_y3=64)
    for splits in (1, 2, 3, 7, 64, 1000):
        out[f"wgrad_splits_{splits}"] = _desc((2, 17, 17, 256, 32, 1, 1, 1, 0, 0), splits=splits)
        out[f"wgrad_taps_splits_{splits}"] = _desc((2, 17, 17, 32, 32, 3, 3, 1, 1, 1), splits=splits)
    return out


def record():
    """Everything tests/golden/conv_dispatch_signatures.json pins."""
    lib = _lib.load()
    out = {"arg_bytes": {"conv": lib.fn_conv2d_arg_bytes(), "wgrad": lib.fn_conv2d_wgrad_arg_bytes()}, "plans": {}}
    for key in PLANS:
        plan = lowered(key)
        out["plans"][key] = plan_signature(lib, plan)
        if key == "v1_train_90":
            out["groups"] = plan_groups(lib, plan)
            out["rejected_groups"] = rejected_groups(lib, plan)
    out["edges"] = {name: descriptor_signature(lib, d) for name, d in edge_descriptors().items()}
    return out


if __name__ == "__main__":      # python -m tests.conv_dispatch_signature OUT.json: record with the library of this checkout
    with open(sys.argv[1], "w") as fh:
        json.dump(record(), fh, indent=1, sort_keys=True)
        fh.write("\n")
