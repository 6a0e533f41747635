"""Times the device spanning tree (fn_mst_*) at the size of the reference's validation set: N = 26 495 unit
rows, E = 512, 530 tight synthetic classes, min_samples 1 and 5.  In one process, alternating:

  spanning_tree_m  the whole Gallery.spanning_tree(m): the top-k search of the core distances (m > 1), fn_mst_init, ceil(log2 N)
                   rounds enqueued at once, the read of info, edges and weights to the host, the host's sort and check;
  rounds_m         fn_mst_init + fn_mst_rounds alone, the core distances given, no host read;
  mates            fn_mate_search without ranks with the arguments of Gallery.leave_one_out_mates(ranks=False): ONE walk of all
                   pairs with two running minima per row.  A round is one such walk with one minimum plus O(N) of contraction, so
                   (rounds run) x this time is the yardstick for `rounds_m`;
  matrix           what a user could do before (--matrix-reps samples, 0 leaves it out): fn_pairwise_sqdist into the [N, N] matrix
                   (2.8 GB), the matrix to the host, scipy.sparse.csgraph.minimum_spanning_tree of its upper triangle.

Every sample is a device-event window (which also spans the host work between its two records) around enough back-to-back calls
to last about 20 ms, after a warm-up of every path; median of --reps samples.  Prints readable lines and, last, one JSON line.

    python tools/bench_hierarchy.py [--reps 7] [--rows 26495] [--matrix-reps 1]"""
import argparse, ctypes, json, sys, time
import numpy as np, torch
sys.path.insert(0, ".")
from facenet_amd import _lib
from facenet_amd.recognize import Gallery

E, CLASSES = 512, 530
ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--rows", type=int, default=26495)
ap.add_argument("--matrix-reps", type=int, default=1)
args = ap.parse_args()
N = args.rows
lib, dev = _lib.load(), torch.device("cuda:0")
stream = lambda: torch.cuda.current_stream(dev).cuda_stream


def window(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e-3 / inner


def bench(paths, reps):
    inner = {}
    for name, fn in paths.items():
        window(fn, 2)
        inner[name] = max(1, min(200, int(0.02 / max(window(fn, 1), 1e-6))))
    samples = {name: [] for name in paths}
    for _ in range(reps):
        for name, fn in paths.items():
            samples[name].append(window(fn, inner[name]))
    return {name: np.array(v) for name, v in samples.items()}, inner


def stats(t):
    return {"median_ms": round(float(np.median(t)) * 1e3, 4), "min_ms": round(float(t.min()) * 1e3, 4), "max_ms": round(float(t.max()) * 1e3, 4)}


gen = torch.Generator(device=dev).manual_seed(1)
unit = lambda x: x / x.norm(dim=1, keepdim=True)
truth = torch.arange(N, device=dev) % CLASSES
rows = unit(unit(torch.randn(CLASSES, E, device=dev, generator=gen))[truth] + 0.3 * torch.randn(N, E, device=dev, generator=gen) / E ** 0.5).contiguous()
gallery = Gallery(rows, labels=truth.cpu().numpy(), device=dev)
skip = torch.arange(N, dtype=torch.int32, device=dev)
MS = (1, 5)
ROUNDS = max(1, int(N - 1).bit_length())
kept, paths = {}, {}

nbytes = ctypes.c_longlong()
_lib.check(lib.fn_mst_workspace(N, 0, ctypes.byref(nbytes)))
ws = torch.empty((nbytes.value + 7) // 8, dtype=torch.int64, device=dev)
comp = torch.empty(N, dtype=torch.int32, device=dev)
edges = torch.empty(N - 1, 2, dtype=torch.int32, device=dev)
weights = torch.empty(N - 1, dtype=torch.float32, device=dev)
info = torch.zeros(8, dtype=torch.int32, device=dev)
core = {m: None if m == 1 else gallery.leave_one_out(m - 1)[0][:, m - 2].contiguous() for m in MS}


def tree_path(m):
    def run():
        kept[f"tree_{m}"] = gallery.spanning_tree(m)
    return run


def rounds_path(m):
    c = None if core[m] is None else core[m].data_ptr()

    def run():
        _lib.check(lib.fn_mst_init(N, comp.data_ptr(), info.data_ptr(), stream()))
        _lib.check(lib.fn_mst_rounds(rows.data_ptr(), N, E, c, 0, ws.data_ptr(), comp.data_ptr(), edges.data_ptr(), weights.data_ptr(),
                                     info.data_ptr(), ROUNDS, stream()))
    return run


for m in MS:
    paths[f"spanning_tree_{m}"] = tree_path(m)
    paths[f"rounds_{m}"] = rounds_path(m)

_lib.check(lib.fn_mate_search_workspace(N, N, 0, ctypes.byref(nbytes)))
mws = torch.empty((nbytes.value + 7) // 8, dtype=torch.int64, device=dev)
mdist = torch.empty(N, 2, dtype=torch.float32, device=dev)
mrows = torch.empty(N, 2, dtype=torch.int32, device=dev)
rng = torch.zeros(2, dtype=torch.int32, device=dev)
codes = truth.to(torch.int32).contiguous()


def mates():
    _lib.check(lib.fn_mate_search(rows.data_ptr(), N, codes.data_ptr(), rows.data_ptr(), N, codes.data_ptr(), E, 0, skip.data_ptr(), 0,
                                  mws.data_ptr(), mdist.data_ptr(), mrows.data_ptr(), None, rng.data_ptr(), stream()))


paths["mates"] = mates
t, inner = bench(paths, args.reps)
med = {name: float(np.median(v)) for name, v in t.items()}
out = {"bench": "hierarchy", "device": torch.cuda.get_device_name(0), "N": N, "E": E, "classes": CLASSES, "reps": args.reps,
       "rounds_enqueued": ROUNDS, "calls_per_window": inner, **{name: stats(v) for name, v in t.items()}}
for name in t:
    print(f"{name:16s} {out[name]}", flush=True)
for m in MS:
    tree = kept[f"tree_{m}"]
    out[f"rounds_run_{m}"] = tree.rounds
    out[f"tree_weight_{m}"] = round(float(tree.weights.astype(np.float64).sum()), 6)
    out[f"rounds_{m}_over_yardstick"] = round(med[f"rounds_{m}"] / (tree.rounds * med["mates"]), 3)
    out[f"spanning_tree_{m}_over_rounds"] = round(med[f"spanning_tree_{m}"] / med[f"rounds_{m}"], 3)
    print(f"min_samples {m}: {tree.rounds} rounds run of {ROUNDS} enqueued; rounds = {out[f'rounds_{m}_over_yardstick']} x (rounds run x mates); "
          f"spanning_tree = {out[f'spanning_tree_{m}_over_rounds']} x rounds; tree weight {out[f'tree_weight_{m}']}", flush=True)

if args.matrix_reps > 0:
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import minimum_spanning_tree
    full = torch.empty(N, N, dtype=torch.float32, device=dev)

    def matrix():
        _lib.check(lib.fn_pairwise_sqdist(rows.data_ptr(), rows.data_ptr(), full.data_ptr(), rng.data_ptr(), N, N, E, 0, stream()))
        d = torch.triu(full, 1).cpu().numpy()
        kept["matrix"] = minimum_spanning_tree(csr_matrix(d))

    samples = []
    for _ in range(args.matrix_reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        matrix()
        samples.append(time.perf_counter() - t0)
        print(f"matrix           {samples[-1] * 1e3:.1f} ms (wall clock, one call)", flush=True)
    mst = kept["matrix"]
    out["matrix"] = stats(np.array(samples))
    out["matrix_reps"] = args.matrix_reps
    out["matrix_edges"] = int(mst.nnz)
    out["matrix_tree_weight"] = round(float(mst.data.astype(np.float64).sum()), 6)
    out["spanning_tree_1_speedup_over_matrix"] = round(float(np.median(samples)) / med["spanning_tree_1"], 1)
    print(f"matrix route: {mst.nnz} edges, tree weight {out['matrix_tree_weight']} (fn_pairwise_sqdist's distances agree with the chain's to "
          f"rounding, not in bits); Gallery.spanning_tree(1) is {out['spanning_tree_1_speedup_over_matrix']} x faster", flush=True)
print(json.dumps(out))
