"""What the center loss and prelogits-norm loss add to a softmax training step: batch 100, E 512,
10 575 classes, bf16, captured graphs.  Two trainers on the same parameters and batch -- regularisers off, and both on --
are timed alternately in one process with device events after a warm-up; prints one JSON line.  The kernels' own times come
from a separate profiler run of the same script with --steps small (rocprofv3 --kernel-trace --stats)."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=100)
    ap.add_argument("--classes", type=int, default=10575)
    ap.add_argument("--steps", type=int, default=20, help="steps per timed window")
    ap.add_argument("--rounds", type=int, default=6, help="alternating windows per configuration")
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    # both trainers on the same convolution tiles: the first one times them, the second reads its choices (otherwise the
    # difference would include two independent tile searches)
    tune = tempfile.NamedTemporaryFile(suffix=".json", delete=False)
    tune.close()
    os.unlink(tune.name)
    os.environ.setdefault("FACENET_TUNE_CACHE", tune.name)
    N, E = a.batch, 512
    rng = np.random.default_rng(0)
    x = torch.from_numpy(rng.integers(0, 256, (N, 160, 160, 3), dtype=np.uint8))
    y = torch.from_numpy(rng.integers(0, a.classes, N))
    params = None
    trainers = {}
    for name, kw in (("off", {}), ("on", dict(center_factor=0.01, prelogits_norm_factor=5e-4))):
        net = Network(embedding_size=E, device="cuda:0", train_dtype=torch.bfloat16, nrof_classes=a.classes, seed=0)
        if params is None:
            params = net.export_keras_params()
        net.load_keras_params(params)
        tr = Trainer(net, batch=N, loss="softmax", lr=0.01, **kw)
        tr.set_images(x, y)
        tr.capture()
        for _ in range(a.warmup):
            tr.step()
        torch.cuda.synchronize()
        trainers[name] = tr
    ms = {k: [] for k in trainers}
    for _ in range(a.rounds):
        for name, tr in trainers.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.steps):
                tr.step()
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1) / a.steps)
    med = {k: statistics.median(v) for k, v in ms.items()}
    terms = trainers["on"].loss_terms()
    print(json.dumps({"batch": N, "embedding": E, "classes": a.classes, "dtype": "bf16", "graph": True,
                      "step_ms_off": round(med["off"], 4), "step_ms_on": round(med["on"], 4),
                      "added_us": round(1000 * (med["on"] - med["off"]), 2),
                      "step_ms_off_all": [round(v, 4) for v in ms["off"]], "step_ms_on_all": [round(v, 4) for v in ms["on"]],
                      "ops_off": len(trainers["off"].step_ops), "ops_on": len(trainers["on"].step_ops),
                      "ops_only_on": sorted({o.name for o in trainers["on"].step_ops} - {o.name for o in trainers["off"].step_ops}),
                      "ops_only_off": sorted({o.name for o in trainers["off"].step_ops} - {o.name for o in trainers["on"].step_ops}),
                      "terms": {k: (None if v is None else round(v, 5)) for k, v in terms.items()}}))


if __name__ == "__main__":
    main()
