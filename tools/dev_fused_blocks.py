"""Developer aid: the fused inference blocks (csrc/block_fused.hip) on their own, the way the mining forward runs them: ten
Block17 launches and five Block35 launches at N = 180, f16, every block with its own weight packs (laid out back to back, each
launch warming the next block's packs through the _warm entry point), ping-ponging between two activation buffers, captured
into one graph per kind and replayed.

    python tools/dev_fused_blocks.py                    the shipped library: us per launch
    FN_DEV_LIB=build/dbg/libfused_phases.so python tools/dev_fused_blocks.py
                                                        a phase-clock build: the per-stage table as well

The phase-clock build is the shipped library with block_fused.hip compiled with -DFN_FUSED_PHASES=1:

    cd facenet_amd/csrc && hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -DFN_FUSED_PHASES=1 -c block_fused.hip -o ../../build/dbg/bf_ph.o &&
    hipcc --offload-arch=gfx950 -shared -fPIC ../../build/dbg/bf_ph.o $(ls ../../build/obj/*.o | grep -v block_fused) -o ../../build/dbg/libfused_phases.so

The table is the mean time (us, 100 MHz wall clock) a workgroup spends between two stamps.  A workgroup is alone on its CU, so
the phases add up to its life; the launch lasts as long as its slowest workgroup plus launch and drain.  The "resid wait" column
drains every outstanding vector-memory request of the wave, so with the LDS-DMA weight stream it also holds what was left of
the two weight tiles in flight (the k-tile column is shorter by as much)."""
import ctypes as C
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from facenet_amd import _lib                              # noqa: E402

if os.environ.get("FN_DEV_LIB"):
    _lib.LIB_PATH = os.path.abspath(os.environ["FN_DEV_LIB"])
lib = _lib.load()

N, REPLAYS = 180, 50
DT = torch.float16
# name -> pack shape, in the argument order of the entry points
B17 = dict(H=8, C=896, n=10, scale=0.10,
           layers=(("t0", (128, 896)), ("t1a", (128, 896)), ("t1b", (128, 7, 128)), ("t1c", (128, 7, 128)), ("up", (896, 256))))
B35 = dict(H=17, C=256, n=5, scale=0.17,
           layers=(("t0", (32, 256)), ("t1a", (32, 256)), ("t2a", (32, 256)), ("t1b", (32, 9, 32)), ("t2b", (32, 9, 32)),
                   ("t2c", (32, 9, 32)), ("up", (256, 96))))
SLOTS17 = ["prologue", "s1 loop", "s1 epi", "s2 loop", "s2 epi", "s3 loop", "s3 epi", "s4 k tiles", "s4 C tile", "s4 resid wait", "s4 stores"]
SLOTS35 = ["prologue", "s1 loop", "s1 epi", "2a stage-in", "2a loop", "2a epi", "2b stage-in", "2b loop", "2b epi", "3 stage-in", "3 loop",
           "3 epi", "s4 stage-in", "s4 k tiles", "s4 C tile", "s4 resid wait", "s4 stores"]


def build(spec):
    """One contiguous weight buffer holding the packs of all blocks (block after block), biases likewise."""
    g = torch.Generator().manual_seed(7)
    per = sum(int(torch.tensor(s).prod()) for _, s in spec["layers"])
    per = (per + 7) // 8 * 8                              # keep every block's range 16-byte aligned
    W = torch.empty(spec["n"] * per, dtype=DT, device="cuda")
    Bs, blocks = [], []
    for b in range(spec["n"]):
        off, wp, bp = b * per, [], []
        for _, shape in spec["layers"]:
            n = int(torch.tensor(shape).prod())
            depth = n // shape[0]
            W[off:off + n] = (torch.randn(n, generator=g) * depth ** -0.5).to(DT).cuda()
            wp.append(W.data_ptr() + off * 2)
            bias = (torch.randn(shape[0], generator=g) * 0.1).cuda()
            Bs.append(bias)
            bp.append(bias.data_ptr())
            off += n
        nxt = (W.data_ptr() + (b + 1) * per * 2, per * 2) if b + 1 < spec["n"] else (None, 0)
        blocks.append((wp, bp, nxt))
    return W, Bs, blocks


def launches(kind, spec, blocks, bufs, keep):
    s = torch.cuda.current_stream().cuda_stream
    for b, (wp, bp, warm) in enumerate(blocks):
        x, y = bufs[b & 1].data_ptr(), bufs[(b + 1) & 1].data_ptr()
        if kind == 17:
            rc = lib.fn_block17_infer_warm(x, y, N, *wp, *bp, spec["scale"], 1, warm[0], warm[1], _lib.FN_F16, s)
        else:
            arr = lambda p: (C.c_void_p * 3)(*p)
            k = (arr(wp[:3]), arr(wp[3:6]), arr(bp[:3]), arr(bp[3:6]))
            keep.append(k)
            rc = lib.fn_block35_infer_warm(x, y, N, k[0], k[1], wp[6], k[2], k[3], bp[6], spec["scale"], 1, warm[0], warm[1], _lib.FN_F16, s)
        _lib.check(rc, f"block{kind} {b}")


def main():
    phases = hasattr(lib, "fn_debug_fused_phases")
    buf = (C.c_ulonglong * 64)()
    if phases:
        lib.fn_debug_fused_phases.restype = C.c_int
        lib.fn_debug_fused_phases.argtypes = [C.c_void_p, C.c_int]
    total = {}
    for kind, spec, names in ((17, B17, SLOTS17), (35, B35, SLOTS35)):
        W, Bs, blocks = build(spec)
        g = torch.Generator().manual_seed(11)
        bufs = [(torch.randn(N, spec["H"], spec["H"], spec["C"], generator=g) * 0.5).to(DT).cuda(), None]
        bufs[1] = torch.empty_like(bufs[0])
        keep = []
        launches(kind, spec, blocks, bufs, keep)          # eager once: LDS opt-in, lazy module load
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            launches(kind, spec, blocks, bufs, keep)
        for _ in range(5):
            graph.replay()
        torch.cuda.synchronize()
        if phases:
            assert lib.fn_debug_fused_phases(None, 1) == 0
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(REPLAYS):
            graph.replay()
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) * 1e3 / REPLAYS / spec["n"]
        total[kind] = us
        print(f"block{kind}: {spec['n']} launches of N = {N} per replay, {REPLAYS} replays: {us:.2f} us per launch", flush=True)
        if phases:
            assert lib.fn_debug_fused_phases(buf, 0) == 0
            t = list(buf)[(0 if kind == 17 else 32):][:32]
            n = max(t[0], 1)
            print(f"  {n} workgroups; mean us per workgroup (the stage-4 columns are sums over its {7 if kind == 17 else 8} passes)")
            tot = 0.0
            for i, name in enumerate(names):
                v = t[1 + i] / n / 100.0
                tot += v
                print(f"  {name:>14s} {v:7.2f}")
            print(f"  {'sum':>14s} {tot:7.2f}")
    return total


if __name__ == "__main__":
    main()
