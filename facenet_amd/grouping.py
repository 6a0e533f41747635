"""Transformations of a launch list before it becomes a schedule: the tile variant of every convolution measured once
(``autotune_convs``), same-level forward / data-gradient convolutions fused into grouped launches (``group_convs``) and the weight
gradients gathered into one grouped launch per tile variant (``group_wgrads``)."""
from __future__ import annotations

import ctypes as C
import json
import os
from typing import Dict, List, Sequence

import torch

from . import _lib
from .engine import Network, _ptr
from .schedule import Op, levelize, region


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
