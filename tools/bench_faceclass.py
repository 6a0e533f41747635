"""Timings of the pair classifiers, one JSON line:
  * the captured training step (fn_f2f_pair_loss_fwd_bwd + Adam) at P = 500 classes x K = 5 rows, E = 512;
  * fn_f2f_pair_counts and the whole ConfusionMatrix at 500 classes x 50 rows, E = 512;
  * the reference's NumPy ConfusionMatrix loop (train_classifier.py:27-39), timed on a subset of classes and extrapolated by
    the number of class pairs.
python tools/bench_faceclass.py [--steps N] [--numpy-classes C]"""
import argparse
import json
import os
import random
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from facenet_amd.apps.train_classifier import ConfusionMatrix, pair_counts  # noqa: E402
from facenet_amd.config import Config  # noqa: E402
from facenet_amd._call import as_table  # noqa: E402
from facenet_amd.faceclass import ClassifierTrainer, FaceToFaceDistanceClassifier, row_norms  # noqa: E402
from facenet_amd.facenet import equal_batches_input_pipeline  # noqa: E402


def classes(C, n, E, seed):
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((C, 1, E)).astype(np.float32)
    c /= np.linalg.norm(c, axis=2, keepdims=True)
    x = c + 0.35 * rng.standard_normal((C, n, E)).astype(np.float32) / np.sqrt(E)
    return [x[i] for i in range(C)]


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps          # microseconds


def numpy_reference(embs, threshold=1.0, theta=1.0):
    """train_classifier.py:27-39 with FaceToFaceDistanceClassifier.predict on NumPy float32 arrays (faceclass.py:45-80)."""
    def distance(x, y):
        y = np.transpose(y)
        norm_x = np.linalg.norm(x, axis=1, keepdims=True)
        norm_y = np.linalg.norm(y, axis=0, keepdims=True)
        return 2 * (1 - (x / norm_x) @ (y / norm_y)) + theta * pow(2 * (norm_x - norm_y) / (norm_x + norm_y), 2)
    s = 0.0
    for i in range(len(embs)):
        for k in range(i):
            s += np.mean(distance(embs[i], embs[k]) < threshold)
        s += np.mean(distance(embs[i], embs[i]) < threshold)
    return s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--numpy-classes", type=int, default=60)
    args = ap.parse_args()
    C, n, E, P, K = 500, 50, 512, 500, 5
    embs = classes(C, n, E, 0)
    out = {"P": P, "K": K, "E": E, "classes": C, "rows_per_class": n}

    model = FaceToFaceDistanceClassifier()
    tr = ClassifierTrainer(model, embs, P, K, learning_rate=1e-4)
    tr.capture()
    random.seed(0)
    rows = next(equal_batches_input_pipeline(embs, Config({"nrof_classes_per_batch": P, "nrof_examples_per_class": K})))
    tr.set_rows(rows)
    for _ in range(20):
        tr.step()
    out["train_step_captured_us"] = round(timed(tr.step, args.steps), 2)
    out["train_step_gflop"] = round(P * K * (P * K - 1) / 2 * 2 * E / 1e9, 3)

    table = as_table(np.concatenate(embs), model.device)
    norms = row_norms(table)
    pair_counts(embs, model, table, norms)
    torch.cuda.synchronize()
    out["pair_counts_us"] = round(timed(lambda: pair_counts(embs, model, table, norms), 5), 1)
    out["pair_counts_gflop"] = round(C * (C + 1) / 2 * n * n * 2 * E / 1e9, 1)
    t0 = time.perf_counter()
    ConfusionMatrix(embs, model)
    out["confusion_matrix_s"] = round(time.perf_counter() - t0, 4)

    m = args.numpy_classes
    t0 = time.perf_counter()
    numpy_reference(embs[:m])
    dt = time.perf_counter() - t0
    out["numpy_reference_subset_classes"] = m
    out["numpy_reference_subset_s"] = round(dt, 3)
    out["numpy_reference_extrapolated_s"] = round(dt * (C * (C + 1) / 2) / (m * (m + 1) / 2), 1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
