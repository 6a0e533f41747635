"""Times the open-set evaluation search (fn_mate_search) on the validation set of section 19 (B): the
leave-one-out self-join Q = G = 26 495, E = 512, 530 classes, unit-norm random rows.  Four paths alternate in one process:

  one_walk      fn_mate_search with rank = NULL: nearest mate and nearest impostor;
  both_walks    fn_mate_search with ranks: the second walk counts the impostors before the mate;
  search_k1     fn_gallery_search at k = 1 with the same skip: the same walk with the top-k epilogue, the yardstick of one_walk;
  matrix        the only route without the kernel: fn_pairwise_sqdist into the [n, n] matrix, two masked torch.min and a masked
                count (its masks are built once, outside the timed windows).

Every sample is a device-event window around enough back-to-back calls to last about 20 ms, after a warm-up of all paths; median,
minimum and maximum of --reps windows.  2 Q G E FLOP per walk against the 157.3 TFLOP/s fp32 MFMA peak.  Prints readable lines
and, last, one JSON line; the same text goes to --out.

    python tools/bench_opensearch.py [--reps 7] [--n 26495] [--classes 530] [--out profiles/opensearch_bench.txt]"""
import argparse, ctypes, json, sys
import numpy as np, torch
sys.path.insert(0, ".")
from facenet_amd import _lib

F32_PEAK = 157.3e12      # MI355X fp32 MFMA
E = 512
ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--n", type=int, default=26495)
ap.add_argument("--classes", type=int, default=530)
ap.add_argument("--out", default="profiles/opensearch_bench.txt")
ap.add_argument("--no-matrix", action="store_true", help="leave the matrix route out (a profiler run of the kernels alone)")
args = ap.parse_args()
lib, dev = _lib.load(), torch.device("cuda:0")
stream = lambda: torch.cuda.current_stream(dev).cuda_stream
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


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
    """paths: name -> callable.  Warm up, size the windows, then alternate the paths `reps` times -> name -> seconds per call."""
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


n, C = args.n, args.classes
gen = torch.Generator(device=dev).manual_seed(1)
x = torch.randn(n, E, device=dev, generator=gen)
x = (x / x.norm(dim=1, keepdim=True)).contiguous()
labels = (torch.arange(n, device=dev) % C).to(torch.int32)[torch.randperm(n, device=dev, generator=gen)].contiguous()
skip = torch.arange(n, dtype=torch.int32, device=dev)
nbytes = ctypes.c_longlong()
_lib.check(lib.fn_mate_search_workspace(n, n, 0, ctypes.byref(nbytes)))
ws = torch.empty((nbytes.value + 7) // 8, dtype=torch.int64, device=dev)
_lib.check(lib.fn_gallery_search_workspace(n, n, 1, 0, ctypes.byref(nbytes)))
ws1 = torch.empty((nbytes.value + 7) // 8, dtype=torch.int64, device=dev)
dist = torch.empty(n, 2, dtype=torch.float32, device=dev)
rows = torch.empty(n, 2, dtype=torch.int32, device=dev)
rank = torch.empty(n, dtype=torch.int32, device=dev)
dist1 = torch.empty(n, 1, dtype=torch.float32, device=dev)
rows1 = torch.empty(n, 1, dtype=torch.int32, device=dev)
rng = torch.zeros(2, dtype=torch.int32, device=dev)
base = {}


def mate_search(rank_ptr):
    _lib.check(lib.fn_mate_search(x.data_ptr(), n, labels.data_ptr(), x.data_ptr(), n, labels.data_ptr(), E, 0, skip.data_ptr(), 0, ws.data_ptr(),
                                  dist.data_ptr(), rows.data_ptr(), rank_ptr, rng.data_ptr(), stream()))


def search_k1():
    _lib.check(lib.fn_gallery_search(x.data_ptr(), n, x.data_ptr(), n, E, 1, 0, skip.data_ptr(), None, 0, ws1.data_ptr(), dist1.data_ptr(),
                                     rows1.data_ptr(), None, rng.data_ptr(), stream()))


paths = {"one_walk": lambda: mate_search(None), "both_walks": lambda: mate_search(rank.data_ptr()), "search_k1": search_k1}
if not args.no_matrix:
    full = torch.empty(n, n, dtype=torch.float32, device=dev)
    same = labels[:, None] == labels[None, :]
    eye = torch.eye(n, dtype=torch.bool, device=dev)
    mate_mask, impostor_mask = same & ~eye, ~same
    del same, eye
    inf = torch.tensor(float("inf"), device=dev)

    def matrix():
        _lib.check(lib.fn_pairwise_sqdist(x.data_ptr(), x.data_ptr(), full.data_ptr(), rng.data_ptr(), n, n, E, 0, stream()))
        base["mate"], base["mate_row"] = torch.where(mate_mask, full, inf).min(dim=1)
        base["impostor"], base["impostor_row"] = torch.where(impostor_mask, full, inf).min(dim=1)
        base["rank"] = ((full < base["mate"][:, None]) & impostor_mask).sum(dim=1)

    paths["matrix"] = matrix

t, inner = bench(paths, args.reps)
mate_search(rank.data_ptr())
search_k1()
torch.cuda.synchronize()
med = {name: float(np.median(v)) for name, v in t.items()}
flop = 2.0 * n * n * E
out = {"bench": "opensearch", "device": torch.cuda.get_device_name(0), "n": n, "E": E, "classes": C, "reps": args.reps, "calls_per_window": inner}
for name in paths:
    out[name] = stats(t[name])
out["one_walk_tflops"] = round(flop / med["one_walk"] / 1e12, 2)
out["one_walk_fraction_of_fp32_mfma_peak"] = round(flop / F32_PEAK / med["one_walk"], 4)
out["both_walks_fraction_of_fp32_mfma_peak"] = round(2 * flop / F32_PEAK / med["both_walks"], 4)
out["one_walk_over_search_k1"] = round(med["one_walk"] / med["search_k1"], 4)
out["one_walk_within_10_percent_of_search_k1"] = med["one_walk"] <= 1.1 * med["search_k1"]
# the nearest other row overall is the nearer of the nearest mate and the nearest impostor: the same key, the same bits
best = torch.where((dist[:, 0] < dist[:, 1]) | ((dist[:, 0] == dist[:, 1]) & (rows[:, 0] < rows[:, 1])), 0, 1)
pick = lambda a: a.gather(1, best[:, None].long())
out["nearest_equals_search_k1"] = bool(torch.equal(pick(rows), rows1) and torch.equal(pick(dist), dist1))
out["rank_zero_share"] = round(float((rank == 0).float().mean()), 6)
say(f"Q = G = {n}, E = {E}, {C} classes, leave-one-out; median [min, max] ms over {args.reps} windows")
for name in paths:
    s = out[name]
    say(f"  {name:<11s} {s['median_ms']:10.4f} [{s['min_ms']:.4f}, {s['max_ms']:.4f}]   ({inner[name]} calls per window)")
say(f"one walk: {out['one_walk_tflops']} TFLOP/s, {out['one_walk_fraction_of_fp32_mfma_peak']} of the fp32 MFMA peak; both walks: "
    f"{out['both_walks_fraction_of_fp32_mfma_peak']}; one walk / search at k = 1: {out['one_walk_over_search_k1']} "
    f"(within 10 %: {out['one_walk_within_10_percent_of_search_k1']}); nearest of (mate, impostor) equals the search's row and "
    f"distance bit for bit: {out['nearest_equals_search_k1']}")
if "matrix" in paths:
    out["matrix_over_one_walk"] = round(med["matrix"] / med["one_walk"], 2)
    out["matrix_over_both_walks"] = round(med["matrix"] / med["both_walks"], 2)
    # the matrix sums its dot products in another order: distances agree to rounding and near-ties may swap
    out["matrix_rows_equal"] = round(float(((base["mate_row"].int() == rows[:, 0]) & (base["impostor_row"].int() == rows[:, 1])).float().mean()), 6)
    out["matrix_ranks_equal"] = round(float((base["rank"].int() == rank).float().mean()), 6)
    out["matrix_max_abs_distance_difference"] = float(torch.maximum((base["mate"] - dist[:, 0]).abs().max(), (base["impostor"] - dist[:, 1]).abs().max()))
    say(f"matrix route / one walk: {out['matrix_over_one_walk']}x, / both walks: {out['matrix_over_both_walks']}x; rows equal to the matrix "
        f"route's {out['matrix_rows_equal']}, ranks {out['matrix_ranks_equal']}, max |distance difference| "
        f"{out['matrix_max_abs_distance_difference']:.3g}")
say(json.dumps(out))
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
