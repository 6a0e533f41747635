"""Times face clustering (fn_radius_count / fn_radius_fill / fn_dbscan_*) at the size of the reference's
validation set: N = 26 495 unit rows, E = 512, 530 tight synthetic classes, eps = 0.5 between the within-class (about 0.17) and
the between-class (about 1.8) distances, min_samples = 1.  In one process, alternating:

  radius        fn_radius_count + fn_radius_fill of the self-join into preallocated rows (no host read in between);
  cluster       the whole Gallery.cluster: count, the read of nnz, fill, the DBSCAN rounds with their flag reads, finish, labels to
                the host;
  leave_one_out fn_gallery_search(k = 1) of the same rows: the same multiply once, with the search's selection.  Each radius pass
                does that multiply without the selection, so twice this time is the yardstick for `radius`;
  matrix        what a user could do before: fn_pairwise_sqdist into the [N, N] matrix (2.8 GB), (D < eps).nonzero(), the pairs
                to the host, scipy.sparse.csgraph.connected_components.

Every sample is a device-event window (which also spans the host work between its two records) around enough back-to-back calls
to last about 20 ms, after a warm-up of every path; median of --reps samples.  Prints readable lines and, last, one JSON line.

    python tools/bench_cluster.py [--reps 7] [--rows 26495]"""
import argparse, ctypes, json, sys
import numpy as np, torch
sys.path.insert(0, ".")
from facenet_amd import _lib
from facenet_amd.recognize import Gallery

F32_PEAK = 157.3e12                       # MI355X fp32 MFMA
E, CLASSES, EPS = 512, 530, 0.5
ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--rows", type=int, default=26495)
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
gallery = Gallery(rows, device=dev)
skip = torch.arange(N, dtype=torch.int32, device=dev)

nbytes = ctypes.c_longlong()
_lib.check(lib.fn_radius_workspace(N, N, 0, ctypes.byref(nbytes)))
ws = torch.empty((nbytes.value + 7) // 8, dtype=torch.int64, device=dev)
offsets = torch.zeros(N + 1, dtype=torch.int64, device=dev)
rng = torch.zeros(2, dtype=torch.int32, device=dev)
common = (rows.data_ptr(), N, rows.data_ptr(), N, E, 0, EPS, skip.data_ptr(), 0, ws.data_ptr())


def count():
    _lib.check(lib.fn_radius_count(*common, offsets.data_ptr(), rng.data_ptr(), stream()))


count()
nnz = int(offsets[N].item())
cols = torch.empty(nnz, dtype=torch.int32, device=dev)
dist = torch.empty(nnz, dtype=torch.float32, device=dev)


def fill():
    _lib.check(lib.fn_radius_fill(*common, cols.data_ptr(), dist.data_ptr(), nnz, stream()))


def radius():
    count()
    fill()


kept = {}


def cluster():
    kept["clustering"] = gallery.cluster(threshold=EPS)


_lib.check(lib.fn_gallery_search_workspace(N, N, 1, 0, ctypes.byref(nbytes)))
sws = torch.empty(nbytes.value // 8, dtype=torch.int64, device=dev)
sdist = torch.empty(N, 1, dtype=torch.float32, device=dev)
srows = torch.empty(N, 1, dtype=torch.int32, device=dev)


def leave_one_out():
    _lib.check(lib.fn_gallery_search(rows.data_ptr(), N, rows.data_ptr(), N, E, 1, 0, skip.data_ptr(), None, 0, sws.data_ptr(), sdist.data_ptr(),
                                     srows.data_ptr(), None, rng.data_ptr(), stream()))


full = torch.empty(N, N, dtype=torch.float32, device=dev)


def matrix():
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import connected_components
    _lib.check(lib.fn_pairwise_sqdist(rows.data_ptr(), rows.data_ptr(), full.data_ptr(), rng.data_ptr(), N, N, E, 0, stream()))
    pairs = (full < EPS).nonzero()
    pairs = pairs[pairs[:, 0] != pairs[:, 1]].cpu().numpy()
    graph = csr_matrix((np.ones(len(pairs), np.int8), (pairs[:, 0], pairs[:, 1])), shape=(N, N))
    kept["matrix"] = (len(pairs), connected_components(graph, directed=False)[1])


t, inner = bench({"count": count, "fill": fill, "radius": radius, "cluster": cluster, "leave_one_out": leave_one_out, "matrix": matrix}, args.reps)
med = {name: float(np.median(v)) for name, v in t.items()}
c = kept["clustering"]
pairs, comp = kept["matrix"]
# the same partition: two labellings agree when the pairs (cluster id, component id) are as many as either side's ids
same = len({(a, b) for a, b in zip(c.labels.tolist(), comp.tolist())}) == c.nrof_clusters == len(set(comp.tolist()))
flop = 2.0 * N * N * E
out = {"bench": "cluster", "device": torch.cuda.get_device_name(0), "N": N, "E": E, "classes": CLASSES, "eps": EPS, "min_samples": 1, "nnz": nnz,
       "clusters": c.nrof_clusters, "noise": c.nrof_noise, "dbscan_rounds": c.rounds, "reps": args.reps, "calls_per_window": inner,
       **{name: stats(v) for name, v in t.items()},
       "radius_over_leave_one_out": round(med["radius"] / med["leave_one_out"], 3),
       "count_over_leave_one_out": round(med["count"] / med["leave_one_out"], 3),
       "fill_over_leave_one_out": round(med["fill"] / med["leave_one_out"], 3),
       "cluster_speedup_over_matrix": round(med["matrix"] / med["cluster"], 2),
       "radius_tflops": round(2 * flop / med["radius"] / 1e12, 2), "radius_fraction_of_fp32_mfma_peak": round(2 * flop / med["radius"] / F32_PEAK, 4),
       "matrix_pairs": pairs, "same_partition_as_matrix_route": bool(same and pairs == nnz)}
for name in t:
    print(f"{name:14s} {out[name]}", flush=True)
print(f"N {N} E {E}: nnz {nnz}, {c.nrof_clusters} clusters, {c.nrof_noise} noise rows, {c.rounds} DBSCAN rounds; radius = "
      f"{out['radius_over_leave_one_out']} x leave_one_out (count {out['count_over_leave_one_out']}, fill {out['fill_over_leave_one_out']}; "
      f"yardstick 2), {out['radius_tflops']} TFLOP/s = {out['radius_fraction_of_fp32_mfma_peak']} of the fp32 MFMA peak; Gallery.cluster "
      f"{out['cluster_speedup_over_matrix']} x faster than the matrix route; same partition: {out['same_partition_as_matrix_route']}", flush=True)
print(json.dumps(out))
sys.exit(0 if out["same_partition_as_matrix_route"] else 1)
