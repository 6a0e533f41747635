"""Times one face-to-face validation pass at the reference's scale (530 classes / 26 489 embeddings of size 512,
models/20200724-231357/logs/report.txt:13-22; 693-1 547 s per pass in the reference's logs, :47,647) on the GPU: the per-fold
path (one fn_confidence_counts launch per training part) and the one-pass path (fn_confidence_counts_folds, DESIGN.md section
16) alternating in one process, each repetition timed with a host clock around work that ends in a device synchronise; and
the NumPy restatement on a bounded sample.

    python tools/bench_validation.py [--reps 5] [--once one_pass|per_fold] [--no-numpy]

``--once PATH`` runs a warm-up and one pass of that path only (for a kernel trace)."""
import argparse, sys, time
import numpy as np, torch
sys.path.insert(0, ".")
from facenet_amd.config import Config
from facenet_amd.statistics import FaceToFaceValidation
from oracle import statistics_oracle as so

def pool(C, per, E, seed=0):
    rng = np.random.default_rng(seed)
    cen = rng.normal(size=(C, 1, E)).astype(np.float32)
    sizes = rng.integers(per[0], per[1] + 1, C)
    emb = np.concatenate([cen[c] * 0.6 + rng.normal(size=(sizes[c], E)).astype(np.float32) * 0.7 for c in range(C)])
    emb /= np.linalg.norm(emb, axis=1, keepdims=True)
    return emb.astype(np.float32), np.repeat(np.arange(C), sizes)

def timed(emb, labels, cfg, one_pass):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    v = FaceToFaceValidation(emb, labels, cfg, one_pass=one_pass)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, v

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--once", choices=("one_pass", "per_fold"), default=None)
ap.add_argument("--no-numpy", action="store_true")
args = ap.parse_args()

emb, labels = pool(530, (49, 51), 512)
print("embeddings", emb.shape, "classes", 530)
cfg = Config({"metric": 0, "nrof_folds": 10, "far_target": 1e-3})
emb_dev = torch.as_tensor(emb).cuda()
if args.once:
    FaceToFaceValidation(emb[:2000], labels[:2000], cfg, one_pass=args.once == "one_pass")
    s, v = timed(emb_dev, labels, cfg, args.once == "one_pass")
    print(f"{args.once}: {s:.3f} s; accuracy {v.dict['MaximumAccuracy']['accuracy']:.5f}")
    sys.exit(0)
for one_pass in (False, True):                                              # warm-up of both paths
    FaceToFaceValidation(emb[:2000], labels[:2000], cfg, one_pass=one_pass)
times, last = {False: [], True: []}, {}
for rep in range(max(5, args.reps)):
    for one_pass in (False, True):
        s, last[one_pass] = timed(emb_dev, labels, cfg, one_pass)
        times[one_pass].append(s)
for one_pass, name in ((False, "per-fold"), (True, "one-pass")):
    t = np.array(times[one_pass])
    print(f"GPU 10-fold validation, {name}: median {np.median(t):.4f} s  min {t.min():.4f}  max {t.max():.4f}  ({len(t)} repetitions); "
          f"accuracy {last[one_pass].dict['MaximumAccuracy']['accuracy']:.5f}  auc {last[one_pass].dict['MaximumAccuracy']['auc']:.7f}")
pf, op = np.array(times[False]), np.array(times[True])
print(f"ratio of medians per-fold / one-pass: {np.median(pf) / np.median(op):.2f}; per-fold spread (max - min) {pf.max() - pf.min():.4f} s; "
      f"difference of medians {np.median(pf) - np.median(op):.4f} s")
n = len(labels)
print(f"pair dot products: n(n-1)/2 * 2E = {n * (n - 1) / 2 * 2 * emb.shape[1]:.4e} FLOP")
if not args.no_numpy:
    e2, l2 = pool(40, (49, 51), 512, seed=1)
    t0 = time.perf_counter(); so.face_to_face_validation(e2, l2, 0, nrof_folds=10); cpu_s = time.perf_counter() - t0
    scale = (530 / 40) ** 2
    print(f"NumPy restatement on 40 classes / {len(l2)} embeddings: {cpu_s:.1f} s  (x{scale:.0f} class pairs at full scale ~ {cpu_s * scale:.0f} s)")
