"""Times the inverted-file index (Gallery.ivf / IVFGallery.search) against the exhaustive search
(fn_gallery_search, section 19) on the same rows in the same run, and reports the recall of the probed search against that
exhaustive answer.  G = 1 048 576 unit rows of E = 512 in tight synthetic classes (the generator of tools/bench_cluster.py),
nlist = 1024, k = 5; the queries are further noisy members of the same classes.

  build    Gallery.ivf(nlist, iters): host clock around the call, ended by a device synchronise (k-means reads counts back)
  search   Q = 16 and Q = 4096, nprobe in {1, 4, 16, 64}: IVFGallery's own path (the centroid search, then fn_ivf_search; no
           normalisation read-back) against fn_gallery_search

All paths of a Q alternate in one process; every sample is a device-event window around enough back-to-back calls to last about
20 ms, after a warm-up of each; the median of --reps windows is reported.  Prints readable lines and, last, one JSON line.

    python tools/bench_ivf.py [--reps 7] [--rows 1048576] [--nlist 1024] [--iters 10]"""
import argparse, json, sys, time
import numpy as np, torch
sys.path.insert(0, ".")
from facenet_amd.recognize import Gallery

E, K, NPROBES = 512, 5, (1, 4, 16, 64)
ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--rows", type=int, default=1 << 20)
ap.add_argument("--nlist", type=int, default=1024)
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--classes", type=int, default=20000)
args = ap.parse_args()
dev = torch.device("cuda:0")
gen = torch.Generator(device=dev).manual_seed(0)


def unit(x):
    return x / x.norm(dim=1, keepdim=True)


def members(centres, n):
    """n noisy unit rows of random classes (within-class distance about 0.17, as in bench_cluster.py)."""
    truth = torch.randint(0, centres.shape[0], (n,), device=dev, generator=gen)
    return unit(centres[truth] + 0.3 * torch.randn(n, E, device=dev, generator=gen) / E ** 0.5).contiguous()


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


centres = unit(torch.randn(args.classes, E, device=dev, generator=gen))
gallery = Gallery(members(centres, args.rows), device=dev)
Gallery(gallery.embeddings[:4096], device=dev).ivf(16, iters=2)          # loads the code objects: not part of the build time
torch.cuda.synchronize()
t0 = time.perf_counter()
index = gallery.ivf(args.nlist, iters=args.iters)
torch.cuda.synchronize()
build_s = time.perf_counter() - t0
lengths = np.diff(index.list_start)
build = {"seconds": round(build_s, 3), "kmeans": index.kmeans_info, "list_rows": {"min": int(lengths.min()), "median": float(np.median(lengths)),
                                                                                  "max": int(lengths.max()), "empty": int((lengths == 0).sum())}}
print(f"build: Gallery.ivf(nlist {args.nlist}, iters {args.iters}) over {args.rows} rows: {build_s:.3f} s; {index.kmeans_info}; "
      f"rows per list min {build['list_rows']['min']} median {build['list_rows']['median']:.0f} max {build['list_rows']['max']}", flush=True)

results = []
for Q in (16, 4096):
    queries = members(centres, Q)
    out = {}
    paths = {"exhaustive": lambda: out.__setitem__("exhaustive", gallery.search(queries, K, atol=None))}
    for nprobe in NPROBES:
        paths[f"ivf_nprobe{nprobe}"] = lambda nprobe=nprobe: out.__setitem__(nprobe, index.search(queries, K, nprobe=nprobe, atol=None))
    t, inner = bench(paths, args.reps)
    full = out["exhaustive"][1]
    te = float(np.median(t["exhaustive"]))
    row = {"Q": Q, "G": args.rows, "E": E, "k": K, "nlist": args.nlist, "reps": args.reps, "calls_per_window": inner,
           "exhaustive": stats(t["exhaustive"]), "ivf": {}}
    print(f"Q {Q}: exhaustive fn_gallery_search {row['exhaustive']}", flush=True)
    for nprobe in NPROBES:
        near = out[nprobe][1]
        recall1 = float((near[:, 0] == full[:, 0]).float().mean())
        recall5 = float((near[:, :, None] == full[:, None, :]).any(dim=2).float().mean())
        ti = float(np.median(t[f"ivf_nprobe{nprobe}"]))
        row["ivf"][nprobe] = dict(stats(t[f"ivf_nprobe{nprobe}"]), speedup=round(te / ti, 2), faster=bool(ti < te), recall_at_1=round(recall1, 6),
                                  recall_at_5=round(recall5, 6))
        print(f"Q {Q} nprobe {nprobe:2d}: {row['ivf'][nprobe]}" + ("" if ti < te else "   NOT faster than the exhaustive search"), flush=True)
    results.append(row)
print(json.dumps({"bench": "ivf", "device": torch.cuda.get_device_name(0), "build": build, "search": results}))
