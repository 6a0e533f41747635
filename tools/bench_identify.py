"""Times 1:N identification (fn_gallery_search) against what a user could do before it existed: the full
distance matrix from fn_pairwise_sqdist followed by torch.topk(k, largest=False).  E = 512, k = 5, unit-norm random rows:

  (A) a photograph's faces: Q = 16 against G = 1 048 576 -- bound by reading the 2 GiB gallery once from HBM;
  (B) leave-one-out over a validation set of the reference's size: Q = G = 26 495 with skip -- bound by the fp32 MFMA rate
      (2 Q G E FLOP against 157.3 TFLOP/s).

Both paths alternate in one process; every sample is a device-event window around enough back-to-back calls to last about 20 ms,
after a warm-up of both.  A plain read of the gallery (torch.sum) is timed the same way as the HBM yardstick of this run.  Prints
a few readable lines and, last, one JSON line.

    python tools/bench_identify.py [--reps 7] [--shape A|B|both]"""
import argparse, ctypes, json, sys
import numpy as np, torch
sys.path.insert(0, ".")
from facenet_amd import _lib

HBM_PEAK, HBM_MEASURED, F32_PEAK = 8.0e12, 6.29e12, 157.3e12      # MI355X: spec, float4 copy, fp32 MFMA
E, K = 512, 5
ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--shape", choices=("A", "B", "both"), default="both")
args = ap.parse_args()
lib, dev = _lib.load(), torch.device("cuda:0")
stream = lambda: torch.cuda.current_stream(dev).cuda_stream


def unit_rows(n, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    x = torch.randn(n, E, device=dev, generator=g)
    return (x / x.norm(dim=1, keepdim=True)).contiguous()


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


def run(shape, Q, G, leave_one_out):
    gallery = unit_rows(G, 1)
    queries = gallery if leave_one_out else unit_rows(Q, 2)
    skip = torch.arange(G, dtype=torch.int32, device=dev) if leave_one_out else None
    nbytes = ctypes.c_longlong()
    _lib.check(lib.fn_gallery_search_workspace(Q, G, K, 0, ctypes.byref(nbytes)))
    ws = torch.empty(nbytes.value // 8, dtype=torch.int64, device=dev)
    dist = torch.empty(Q, K, dtype=torch.float32, device=dev)
    rows = torch.empty(Q, K, dtype=torch.int32, device=dev)
    rng = torch.zeros(2, dtype=torch.int32, device=dev)
    kb = K + 1 if leave_one_out else K                       # the baseline drops the row itself after the sort
    full = torch.empty(Q, G, dtype=torch.float32, device=dev)
    base = {}

    def new():
        _lib.check(lib.fn_gallery_search(queries.data_ptr(), Q, gallery.data_ptr(), G, E, K, 0, None if skip is None else skip.data_ptr(), None, 0,
                                         ws.data_ptr(), dist.data_ptr(), rows.data_ptr(), None, rng.data_ptr(), stream()))

    def baseline():
        _lib.check(lib.fn_pairwise_sqdist(queries.data_ptr(), gallery.data_ptr(), full.data_ptr(), rng.data_ptr(), Q, G, E, 0, stream()))
        base["d"], base["i"] = torch.topk(full, kb, dim=1, largest=False)

    def read():
        base["sum"] = gallery.sum()

    t, inner = bench({"gallery_search": new, "matrix_topk": baseline, "read_gallery": read}, args.reps)
    # the two paths sum the dot product in different orders, so distances agree to rounding and near-ties may swap
    bi, bd = base["i"], base["d"]
    if leave_one_out:
        keep = bi != torch.arange(Q, device=dev)[:, None]
        first = keep.long().cumsum(1) <= K
        pick = (keep & first)
        bi, bd = bi[pick].view(Q, -1)[:, :K], bd[pick].view(Q, -1)[:, :K]
    same = float((bi.int() == rows).float().mean())
    ddiff = float((bd - dist).abs().max())
    flop, gbytes = 2.0 * Q * G * E, float(G) * E * 4
    tn, tb, tr = (float(np.median(t[n])) for n in ("gallery_search", "matrix_topk", "read_gallery"))
    floor = max(flop / F32_PEAK, gbytes / HBM_PEAK)
    out = {"shape": shape, "Q": Q, "G": G, "E": E, "k": K, "skip": leave_one_out, "reps": args.reps, "calls_per_window": inner,
           "gallery_search": stats(t["gallery_search"]), "matrix_topk": stats(t["matrix_topk"]), "read_gallery": stats(t["read_gallery"]),
           "speedup": round(tb / tn, 2), "bound": "fp32 MFMA" if flop / F32_PEAK > gbytes / HBM_PEAK else "HBM",
           "roofline_fraction": round(floor / tn, 4), "gallery_bytes_per_s": round(gbytes / tn / 1e12, 3),
           "fraction_of_hbm_peak_8TBs": round(gbytes / tn / HBM_PEAK, 4), "fraction_of_hbm_measured_6.29TBs": round(gbytes / tn / HBM_MEASURED, 4),
           "fraction_of_plain_read_this_run": round(tr / tn, 4), "tflops": round(flop / tn / 1e12, 2),
           "rows_equal_to_baseline": round(same, 6), "max_abs_distance_difference": ddiff}
    print(f"({shape}) Q {Q} G {G}: gallery_search {out['gallery_search']}  matrix+topk {out['matrix_topk']}  speedup {out['speedup']}x; "
          f"{out['tflops']} TFLOP/s, gallery read at {out['gallery_bytes_per_s']} TB/s (plain read {gbytes / tr / 1e12:.2f} TB/s); "
          f"{out['bound']}-bound roofline fraction {out['roofline_fraction']}; rows equal to the baseline's {same:.6f}, "
          f"max |distance difference| {ddiff:.3g}", flush=True)
    return out


results = []
if args.shape in ("A", "both"):
    results.append(run("A", 16, 1 << 20, False))
    torch.cuda.empty_cache()
if args.shape in ("B", "both"):
    results.append(run("B", 26495, 26495, True))
ok = all(r["speedup"] > 1 for r in results)
print(json.dumps({"bench": "identify", "device": torch.cuda.get_device_name(0), "faster_than_baseline_everywhere": ok, "shapes": results}))
sys.exit(0 if ok else 1)
