"""What the moving average of the weights costs.

1. The optimiser pass alone: fn_adam_keras against fn_adam_keras_ema on buffers of the real parameter counts -- the v1
   triplet network (E 128) and softmax training (E 512, 10 575 classes) -- with achieved bytes/s and the share of the HBM
   peak.  Bytes are what the pass must move: fn_adam_keras reads w, g, m, v and writes w, m, v (28 B per parameter) plus the
   2-byte training pack; the fused entry also reads and writes the shadow (+8 B).
2. The captured training step of the bench workload (v1, E 128, triplet batch 90, bf16) with the feature off and on.

Both comparisons alternate A and B in one process, timed with HIP events: 20 warm-up launches (steps) of each, then 10
alternating windows of 20 (200 timed per variant).  Prints one JSON line."""
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
from facenet_amd import _lib                    # noqa: E402
from facenet_amd.engine import Network          # noqa: E402
from facenet_amd.train import Trainer           # noqa: E402

HBM_PEAK = 8.0e12          # bytes/s, MI355X HBM3E specification


def _ptr(t):
    return t.data_ptr()


def alternate(fns, warmup, windows, per_window):
    """{name: [ms per call of each window]}: every fn warmed up, then the windows alternate between them."""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(windows):
        for name, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(per_window):
                fn()
            b.record()
            b.synchronize()
            out[name].append(a.elapsed_time(b) / per_window)
    return out


def optimizer_pass(lib, label, net, warmup, windows, per_window):
    n, n_lp, n_decay = net.n_params, net.n_kernel, net.n_decay
    g = torch.Generator(device="cuda").manual_seed(0)
    w = torch.randn(n, device="cuda", generator=g) * 0.05
    grad = torch.randn(n, device="cuda", generator=g) * 1e-3
    m, v = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    shadow = w.clone()
    w_lp = torch.zeros(n_lp, dtype=torch.bfloat16, device="cuda")
    hyper = torch.tensor([1e-4, 0.9, 0.999, 1.0, 0.0, 0.0, 0.0, 0.0], device="cuda")
    hyper.view(torch.int32)[4:5].fill_(1000)
    st = torch.cuda.current_stream().cuda_stream
    args = (_ptr(w), _ptr(grad), _ptr(m), _ptr(v), _ptr(w_lp), n_lp, n, n_decay, _ptr(hyper), 0.9, 0.999, 0.1, 5e-4, _lib.FN_BF16)
    fns = {"adam_keras": lambda: _lib.check(lib.fn_adam_keras(*args, st), "adam_keras"),
           "adam_keras_ema": lambda: _lib.check(lib.fn_adam_keras_ema(*args, _ptr(shadow), 0.9999, st), "adam_keras_ema")}
    ms = alternate(fns, warmup, windows, per_window)
    nbytes = {"adam_keras": 28.0 * n + 2.0 * n_lp, "adam_keras_ema": 36.0 * n + 2.0 * n_lp}
    res = {"params": n}
    for k, times in ms.items():
        t = statistics.median(times) * 1e-3
        res[k] = {"us": round(t * 1e6, 2), "us_windows": [round(x * 1e3, 2) for x in times], "bytes": nbytes[k],
                  "tb_per_s": round(nbytes[k] / t / 1e12, 3), "hbm_peak_share": round(nbytes[k] / t / HBM_PEAK, 3)}
    res["added_us"] = round(res["adam_keras_ema"]["us"] - res["adam_keras"]["us"], 2)
    return label, res


def training_step(warmup, windows, per_window):
    tune = tempfile.NamedTemporaryFile(suffix=".json", delete=False)     # both trainers on the same convolution tiles
    tune.close()
    os.unlink(tune.name)
    os.environ.setdefault("FACENET_TUNE_CACHE", tune.name)
    B = 90
    x = torch.from_numpy(np.random.default_rng(0).integers(0, 256, (B, 160, 160, 3), dtype=np.uint8))
    params, fns, trainers = None, {}, []
    for name, decay in (("off", None), ("on", 0.9999)):
        net = Network(embedding_size=128, device="cuda:0", train_dtype=torch.bfloat16, infer_dtype=torch.float16, seed=0)
        if params is None:
            params = net.export_keras_params()
        net.load_keras_params(params)
        tr = Trainer(net, batch=B, loss="triplet", alpha=0.2, lr=0.05, moving_average_decay=decay)
        tr.set_images(x)
        tr.capture()
        trainers.append(tr)
        fns[name] = tr.step
    ms = alternate(fns, warmup, windows, per_window)
    off, on = statistics.median(ms["off"]), statistics.median(ms["on"])
    return {"batch": B, "off_ms": round(off, 4), "on_ms": round(on, 4), "added_us": round((on - off) * 1e3, 2),
            "added_pct": round(100.0 * (on - off) / off, 3), "off_windows_ms": [round(t, 4) for t in ms["off"]],
            "on_windows_ms": [round(t, 4) for t in ms["on"]], "launches": [len(t.step_ops) for t in trainers]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--windows", type=int, default=10)
    ap.add_argument("--per-window", type=int, default=20)
    ap.add_argument("--skip-step", action="store_true", help="time the optimiser pass only")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    lib = _lib.load()
    out = {"kernel": dict(optimizer_pass(lib, label, net, a.warmup, a.windows, a.per_window) for label, net in (
        ("v1_triplet_e128", Network(embedding_size=128, allocate=False)),
        ("softmax_e512_c10575", Network(embedding_size=512, nrof_classes=10575, allocate=False))))}
    if not a.skip_step:
        out["step"] = training_step(a.warmup, a.windows, a.per_window)
    line = json.dumps(out)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
