"""Times the false examples (fn_false_pairs + FalseExamples) at the size sections 16 and 23 quote: 26 495
embeddings in 530 classes, E = 512 (the pool of tools/bench_verification.py), at two thresholds: the mean max-accuracy threshold of
the k-fold report and the exact threshold of FAR = 1e-3 (VerificationCurve).

  - device time of fn_false_pairs at each threshold and, alternating with it in the same windows, of one fn_pair_key_histogram
    pass (the first pass's eight octave windows): the yardstick, one walk of the same pairs;
  - the end-to-end time of FalseExamples(...) on the host clock (it ends in a read-back) and what it found;
  - the route of the reference: per pair of classes ``emb_a @ emb_b.T`` -> distances -> argmin / exclude, per class the argmax
    loop, with torch on the device, over a sample of the pairs of classes and extrapolated to all of them.

Prints a few readable lines and, last, one JSON line.

    python tools/bench_false_examples.py [--reps 7] [--sample 2000]"""
import argparse, ctypes, json, sys, time
import numpy as np, torch
sys.path.insert(0, ".")
from facenet_amd import _lib
from facenet_amd import statistics as st
from facenet_amd.config import Config

N, C, E = 26495, 530, 512
ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--sample", type=int, default=2000)
ap.add_argument("--noise", type=float, default=0.6)
args = ap.parse_args()
lib, dev = _lib.load(), torch.device("cuda:0")
MAX_FNEG, MAX_FPOS = 10, 2


def embeddings(seed=0):          # tools/bench_verification.py's
    rng = np.random.default_rng(seed)
    labels = np.sort(np.arange(N) % C)
    centres = rng.normal(size=(C, E))
    centres /= np.linalg.norm(centres, axis=1, keepdims=True)
    noise = rng.normal(size=(N, E))
    x = centres[labels] + args.noise * noise / np.linalg.norm(noise, axis=1, keepdims=True)
    x = (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
    p = rng.permutation(N)
    return x[p], labels[p]


def window(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / inner


def stats(t):
    t = np.asarray(t)
    return {"median_ms": round(float(np.median(t)), 4), "min_ms": round(float(t.min()), 4), "max_ms": round(float(t.max()), 4)}


x, labels = embeddings()
x_dev = torch.from_numpy(x).to(dev)

# ---- the two thresholds ---------------------------------------------------------------------------------------------------------------
report = st.FaceToFaceValidation(x_dev, labels, Config({"metric": 0, "nrof_folds": 10, "far_target": 1e-3}), device=str(dev))
curve = st.VerificationCurve(x_dev, labels, device=str(dev))
thresholds = {"max accuracy": float(np.mean([m.threshold for m in report.reports[0].conf_matrix_test])),
              "FAR 1e-3": curve.threshold_at_far(1e-3)}
print(f"{N} embeddings, {C} classes, E {E}: {curve.nrof_genuine} genuine and {curve.nrof_impostor} impostor pairs, "
      f"{C * (C - 1) // 2} pairs of classes", flush=True)

# ---- device time: fn_false_pairs at each threshold and one histogram pass, alternating ---------------------------------------------------
emb, cls = curve._emb, curve._cls
capacity = 1 << 20
buf = torch.zeros(4 + 2 * capacity, dtype=torch.int64, device=dev)
hist = torch.zeros(8 * 2 * (st.KEY_BINS + 2), dtype=torch.int64, device=dev)
rng_words = torch.zeros(2, dtype=torch.int32, device=dev)
stream = torch.cuda.current_stream(dev).cuda_stream
lo, shift = st.FIRST_WINDOWS
lo_a, sh_a = (ctypes.c_uint32 * 8)(*lo), (ctypes.c_int32 * 8)(*shift)


def false_pairs(t):
    def run():
        buf[:4].zero_()
        _lib.check(lib.fn_false_pairs(emb.data_ptr(), cls.data_ptr(), C, E, 0, t, MAX_FNEG, MAX_FPOS, buf.data_ptr() + 32, capacity,
                                      buf.data_ptr(), buf.data_ptr() + 16, stream))
    return run


def histogram():
    _lib.check(lib.fn_pair_key_histogram(emb.data_ptr(), cls.data_ptr(), C, E, 0, lo_a, sh_a, 8, hist.data_ptr(), rng_words.data_ptr(), stream))


timed = {f"fn_false_pairs at {name} ({t:.5f})": false_pairs(t) for name, t in thresholds.items()}
timed["fn_pair_key_histogram, first pass (R 8, shift 13)"] = histogram
samples = {name: [] for name in timed}
for fn in timed.values():
    window(fn, 2)
for _ in range(args.reps):
    for name, fn in timed.items():
        samples[name].append(window(fn, 3))
kernel_ms = {name: stats(v) for name, v in samples.items()}
yard = kernel_ms["fn_pair_key_histogram, first pass (R 8, shift 13)"]["median_ms"]
for name, s in kernel_ms.items():
    print(f"  {name}: {s}  ({s['median_ms'] / yard:.2f} x the histogram pass)", flush=True)

# ---- end to end -----------------------------------------------------------------------------------------------------------------------
found, e2e = {}, {}
for name, t in thresholds.items():
    times = []
    for _ in range(args.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f = st.FalseExamples(x_dev, labels, t, max_fneg=MAX_FNEG, max_fpos=MAX_FPOS, device=str(dev))
        times.append((time.perf_counter() - t0) * 1e3)
    found[name] = {"threshold": t, "false_negatives": f.nrof_false_negatives, "false_positives": f.nrof_false_positives}
    e2e[name] = stats(times)
    print(f"  FalseExamples at {name}: {found[name]}; end to end {e2e[name]}", flush=True)

# ---- the reference's route over a sample of the pairs of classes ---------------------------------------------------------------------------
order = np.argsort(labels, kind="stable")
xs = x_dev[torch.from_numpy(order).to(dev)]
starts = np.concatenate([[0], np.cumsum(np.bincount(labels, minlength=C))])
rs = np.random.default_rng(1)
a_s = rs.integers(0, C - 1, args.sample)
b_s = np.array([rs.integers(a + 1, C) for a in a_s])


def matrix_route(t):
    torch.cuda.synchronize()
    t0, picks = time.perf_counter(), 0
    for a, b in zip(a_s, b_s):
        d = 2 * (1 - (xs[starts[a]:starts[a + 1]] @ xs[starts[b]:starts[b + 1]].T).clamp(-1, 1))
        for _ in range(MAX_FPOS):
            flat = int(torch.argmin(d))
            i, k = divmod(flat, d.shape[1])
            if not float(d[i, k]) < t:
                break
            picks += 1
            d[i, :] = float("inf")
            d[:, k] = float("inf")
    torch.cuda.synchronize()
    off = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    for c in range(C):
        rows = xs[starts[c]:starts[c + 1]]
        d = torch.triu(2 * (1 - (rows @ rows.T).clamp(-1, 1)), diagonal=1) - torch.tril(torch.ones(len(rows), len(rows), device=dev))
        for _ in range(MAX_FNEG):
            flat = int(torch.argmax(d))
            i, k = divmod(flat, d.shape[1])
            if not float(d[i, k]) > t:
                break
            picks += 1
            d[[i, k], :] = -1
            d[:, [i, k]] = -1
    torch.cuda.synchronize()
    diag = (time.perf_counter() - t0) * 1e3
    return off, diag, picks


matrix_route(thresholds["max accuracy"])          # warm
route = {}
for name, t in thresholds.items():
    off, diag, picks = matrix_route(t)
    total = off * (C * (C - 1) // 2) / args.sample + diag
    route[name] = {"sampled_pairs_of_classes": args.sample, "sample_ms": round(off, 1), "classes_ms": round(diag, 1),
                   "extrapolated_ms": round(total, 1), "picks_in_sample": picks}
    print(f"  matrix route at {name}: {route[name]}", flush=True)

print(json.dumps({"bench": "false_examples", "device": torch.cuda.get_device_name(0), "N": N, "classes": C, "E": E, "noise": args.noise,
                  "max_fneg": MAX_FNEG, "max_fpos": MAX_FPOS, "thresholds": thresholds, "kernel_ms": kernel_ms, "found": found,
                  "end_to_end_ms": e2e, "matrix_route": route}))
