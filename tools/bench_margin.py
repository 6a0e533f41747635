"""What the margin-softmax head costs: the loss ops of a softmax trainer with and without it at the
reference's shape -- batch 100, E 512, 10 575 classes, bf16.  After one forward pass the loss ops alone are replayed eagerly
between device events (back to back: operands that fit stay in the Infinity Cache), and each of the three new launches is timed
on its own both back to back and from cold caches (after a 512 MiB write to another buffer), with the bytes it moves and the
rate that makes.  A single launch between two events includes the events' own few microseconds.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import tempfile
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from facenet_amd.engine import Network          # noqa: E402
from facenet_amd.train import Trainer           # noqa: E402

NEW = ("margin_rnorm", "margin_softmax", "margin_wgrad_fix")


def timed(fn, reps, before=None):
    """Median device time of fn() in microseconds; before() runs ahead of every timed call, outside the events."""
    us = []
    for _ in range(reps):
        if before is not None:
            before()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        us.append(1000 * e0.elapsed_time(e1))
    return statistics.median(us)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=100)
    ap.add_argument("--classes", type=int, default=10575)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--burst", type=int, default=20, help="back-to-back launches per timed window")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    tune = tempfile.NamedTemporaryFile(suffix=".json", delete=False)       # both trainers on the same convolution tiles
    tune.close()
    os.unlink(tune.name)
    os.environ.setdefault("FACENET_TUNE_CACHE", tune.name)
    N, E, C = a.batch, 512, a.classes
    rng = np.random.default_rng(0)
    x = torch.from_numpy(rng.integers(0, 256, (N, 160, 160, 3), dtype=np.uint8))
    y = torch.from_numpy(rng.integers(0, C, N))
    scratch = torch.empty(512 << 20, dtype=torch.uint8, device="cuda")
    out, params = {"batch": N, "embedding": E, "classes": C, "dtype": "bf16"}, None
    for name, kw in (("plain", {}), ("margin", dict(margin_scale=64.0, margin_arc=0.5))):
        net = Network(embedding_size=E, device="cuda:0", train_dtype=torch.bfloat16, nrof_classes=C, seed=0)
        if params is None:
            params = net.export_keras_params()
        net.load_keras_params(params)
        tr = Trainer(net, batch=N, loss="softmax", lr=0.01, **kw)
        tr.set_images(x, y)
        st = net.stream()
        tr._zero()
        tr.plan.run_ops(tr.plan.fwd, st)
        run = lambda ops: tr.plan.run_ops(ops, st)
        for _ in range(3):
            run(tr.loss_ops)
        torch.cuda.synchronize()
        out[f"loss_ops_{name}"] = [op.name for op in tr.loss_ops]
        out[f"loss_ops_us_{name}"] = round(timed(lambda: [run(tr.loss_ops) for _ in range(a.burst)], a.reps) / a.burst, 2)
        out[f"loss_ops_cold_us_{name}"] = round(timed(lambda: run(tr.loss_ops), a.reps, before=lambda: scratch.fill_(1)), 2)
        out[f"loss_{name}"] = round(tr.loss_value(), 5)
        if name == "margin":
            Cp = net.layers["classifier/logits"].cout
            nbytes = {"margin_rnorm": C * E * 4 + C * 4,                                     # the class rows once, the norms out
                      "margin_softmax": N * C * 4 + C * 4 + N * Cp * 2 + 2 * C * 8,         # logits once (re-read from cache), rnorm, dz out, t
                      "margin_wgrad_fix": 3 * C * E * 4 + C * 4 + 2 * C * 8}                 # dw in and out, the class rows in, rnorm, t
            for op in tr.loss_ops:
                if op.name in NEW:
                    warm = timed(lambda: [run([op]) for _ in range(a.burst)], a.reps) / a.burst
                    cold = timed(lambda: run([op]), a.reps, before=lambda: scratch.fill_(1))
                    out[op.name] = {"bytes": nbytes[op.name], "us_back_to_back": round(warm, 2), "us_cold": round(cold, 2),
                                    "GBps_back_to_back": round(nbytes[op.name] / warm / 1e3, 1), "GBps_cold": round(nbytes[op.name] / cold / 1e3, 1)}
        del tr, net
    out["added_us"] = round(out["loss_ops_us_margin"] - out["loss_ops_us_plain"], 2)
    out["added_cold_us"] = round(out["loss_ops_cold_us_margin"] - out["loss_ops_cold_us_plain"], 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
