"""Times the exact verification curve (fn_pair_key_histogram + VerificationCurve) at the size sections 16 and
19 quote: 26 495 embeddings in 530 classes, E = 512, seeded class centres plus noise, renormalised; FAR targets 1e-2, 1e-3, 1e-4,
1e-6 and the EER.

  - device time of every pass of the descent (device events around back-to-back launches of that pass's windows), and of one
    window that is linear in the key over the whole range, the first pass the octave windows replace;
  - the number of passes, and the end-to-end time of tar_at_far + eer on the host clock (the calls end in a read-back);
  - the baseline, what a user could do before: the distance matrix in row blocks through pairwise_similarities, the impostor
    distances gathered on the device, torch.kthvalue per target.  fn_pairwise_sqdist sums its dot products in another order, so
    its thresholds agree with the curve's to rounding; the largest difference is reported.

Prints a few readable lines and, last, one JSON line.

    python tools/bench_verification.py [--reps 7] [--no-baseline]"""
import argparse, ctypes, json, sys, time
from fractions import Fraction
import numpy as np, torch
sys.path.insert(0, ".")
from facenet_amd import _lib
from facenet_amd import statistics as st

N, C, E = 26495, 530, 512
FARS = [1e-6, 1e-4, 1e-3, 1e-2]
FOLDS_KERNEL_MS = 12.6            # fn_confidence_counts_folds at this size (README): the same dot products, two LDS atomics per pair
ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--no-baseline", action="store_true")
ap.add_argument("--noise", type=float, default=0.6)
args = ap.parse_args()
lib, dev = _lib.load(), torch.device("cuda:0")


def embeddings(seed=0):
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

# ---- the curve, once, recording every pass's windows ---------------------------------------------------------------------------------
curve = st.VerificationCurve(x_dev, labels, device=str(dev))
passes = []
inner_hist = curve._histogram
curve._histogram = lambda lo, shift: (passes.append((list(lo), list(shift))), inner_hist(lo, shift))[1]
records = curve.tar_at_far(FARS)
eer = curve.eer()
auc = curve.auc()
print(f"{N} embeddings, {C} classes, E {E}: {curve.nrof_genuine} genuine and {curve.nrof_impostor} impostor pairs; "
      f"{curve.nrof_passes} passes for {len(FARS)} FAR targets and the EER", flush=True)
for r in records:
    print("  FAR target {far_target:g}: threshold {threshold:.7f}, false accepts {false_accepts}, TAR {tar:.6f}".format(**r))
print("  EER {eer:.6f} at {eer_threshold:.7f}; AUC {0:.9f} in [{1:.9f}, {2:.9f}]".format(*auc, **eer), flush=True)

# ---- device time per pass -------------------------------------------------------------------------------------------------------------
out = torch.zeros(8 * 2 * (st.KEY_BINS + 2), dtype=torch.int64, device=dev)
rng_words = torch.zeros(2, dtype=torch.int32, device=dev)


def launcher(lo, shift):
    R = len(lo)
    lo_a, sh_a = (ctypes.c_uint32 * R)(*lo), (ctypes.c_int32 * R)(*shift)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def run():
        _lib.check(lib.fn_pair_key_histogram(curve._emb.data_ptr(), curve._cls.data_ptr(), C, E, 0, lo_a, sh_a, R, out.data_ptr(),
                                             rng_words.data_ptr(), stream))
    return run


timed = {f"pass {k + 1} (R {len(lo)}, shift {min(shift)}..{max(shift)})": launcher(lo, shift) for k, (lo, shift) in enumerate(passes)}
timed["one linear window over [0, 4] (R 1, shift 21)"] = launcher([0], [21])
samples = {name: [] for name in timed}
for fn in timed.values():
    window(fn, 2)
for _ in range(args.reps):
    for name, fn in timed.items():
        samples[name].append(window(fn, 3))
pass_ms = {name: stats(v) for name, v in samples.items()}
for name, s in pass_ms.items():
    print(f"  {name}: {s}  ({s['median_ms'] / FOLDS_KERNEL_MS:.2f} x the {FOLDS_KERNEL_MS} ms of fn_confidence_counts_folds)", flush=True)

# ---- end to end -----------------------------------------------------------------------------------------------------------------------
def end_to_end():
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    c = st.VerificationCurve(x_dev, labels, device=str(dev))
    t1 = time.perf_counter()
    got = c.tar_at_far(FARS), c.eer()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    assert got == (records, eer)
    return (t1 - t0) * 1e3, (t2 - t1) * 1e3


e2e = np.array([end_to_end() for _ in range(args.reps)])
build_ms, answer_ms = stats(e2e[:, 0]), stats(e2e[:, 1])
print(f"  end to end: VerificationCurve(...) {build_ms}; tar_at_far + eer {answer_ms}", flush=True)

# ---- the baseline ---------------------------------------------------------------------------------------------------------------------
baseline = None
if not args.no_baseline:
    order = np.argsort(labels, kind="stable")
    xs, ls = x[order], torch.from_numpy(labels[order]).to(dev)
    ranks = [int(Fraction(f) * curve.nrof_impostor) for f in FARS]

    def matrix_kthvalue():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        impostor = torch.empty(curve.nrof_impostor, dtype=torch.float32, device=dev)
        at, rows = 0, torch.arange(N, device=dev)
        for r0 in range(0, N, 2048):
            d = torch.from_numpy(st.pairwise_similarities(xs[r0:r0 + 2048], xs, metric=0, device=str(dev))).to(dev)
            keep = (ls[r0:r0 + 2048, None] != ls[None, :]) & (rows[None, :] > rows[r0:r0 + 2048, None])
            picked = d[keep]
            impostor[at:at + picked.numel()] = picked
            at += picked.numel()
        assert at == curve.nrof_impostor
        thresholds = [float(torch.kthvalue(impostor, m + 1).values) for m in ranks]
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, thresholds

    runs = [matrix_kthvalue() for _ in range(2)]
    diff = max(abs(t - r["threshold"]) for t, r in zip(runs[-1][1], records))
    baseline = {"ms": [round(r[0], 1) for r in runs], "max_abs_threshold_difference": diff}
    print(f"  baseline (matrix in row blocks through pairwise_similarities, impostors gathered, torch.kthvalue x {len(FARS)}): "
          f"{baseline['ms']} ms (first run cold); largest |threshold difference| {diff:.3g}", flush=True)

print(json.dumps({"bench": "verification", "device": torch.cuda.get_device_name(0), "N": N, "classes": C, "E": E, "noise": args.noise,
                  "far_targets": FARS, "nrof_genuine": curve.nrof_genuine, "nrof_impostor": curve.nrof_impostor, "passes": curve.nrof_passes,
                  "windows": [{"R": len(lo), "shift": shift} for lo, shift in passes], "pass_ms": pass_ms,
                  "confidence_counts_folds_ms_readme": FOLDS_KERNEL_MS, "construct_ms": build_ms, "tar_at_far_plus_eer_ms": answer_ms,
                  "records": records, "eer": eer, "auc": auc, "baseline": baseline}))
sys.exit(0 if baseline is None or baseline["max_abs_threshold_difference"] <= 1e-5 else 1)
