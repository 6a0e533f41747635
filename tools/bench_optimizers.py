"""What the update rules of train.optimizer cost.

1. The optimiser pass alone, for every rule with and without the moving average: fn_adam_keras(_ema) for ADAM, fn_opt_keras(_ema)
   for the others, on buffers of the real parameter counts -- the v1 triplet network (E 128) and softmax training (E 512,
   10 575 classes).  Bytes are what the pass must move: w and every slot read and written, g read (4 B each), plus the 2-byte
   training pack of the kernels; the moving average reads and writes the shadow (+8 B).  Reported against the 6.29 TB/s that a
   float4 copy reaches on the MI355X (MI355X_MICROARCH.md).
2. The captured training step of v1 softmax training (E 512, 10 575 classes, batch 90, bf16) under every rule.

Each comparison alternates its variants in one process, timed with HIP events: warm-up launches (steps) of each, then
alternating windows (median of the windows).  Prints one JSON line."""
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
from facenet_amd import _lib                            # noqa: E402
from facenet_amd.engine import Network                  # noqa: E402
from facenet_amd.train import OPTIMIZERS, Trainer       # noqa: E402

COPY_RATE = 6.29e12        # bytes/s, float4 copy measured on the MI355X


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


def optimizer_pass(lib, net, warmup, windows, per_window):
    n, n_lp, n_decay = net.n_params, net.n_kernel, net.n_decay
    g = torch.Generator(device="cuda").manual_seed(0)
    w = torch.randn(n, device="cuda", generator=g) * 0.05
    grad = torch.randn(n, device="cuda", generator=g) * 1e-3
    s1, s2 = torch.full((n,), 0.1, device="cuda"), torch.zeros(n, device="cuda")
    shadow = w.clone()
    w_lp = torch.zeros(n_lp, dtype=torch.bfloat16, device="cuda")
    hyper = torch.tensor([1e-4, 0.9, 0.999, 1.0, 0.0, 0.0, 0.0, 0.0], device="cuda")
    hyper.view(torch.int32)[4:5].fill_(1000)
    st = torch.cuda.current_stream().cuda_stream
    p = lambda t: t.data_ptr()
    fns, nbytes = {}, {}
    for name, r in OPTIMIZERS.items():
        if name == "ADAM":
            args = (p(w), p(grad), p(s1), p(s2), p(w_lp), n_lp, n, n_decay, p(hyper), 0.9, 0.999, 0.1, 5e-4, _lib.FN_BF16)
            plain, fused = lib.fn_adam_keras, lib.fn_adam_keras_ema
        else:
            args = (r.code, p(w), p(grad), p(s1), p(s2) if len(r.slots) > 1 else None, p(w_lp), n_lp, n, n_decay, p(hyper), r.rho,
                    r.momentum, r.epsilon, 5e-4, _lib.FN_BF16)
            plain, fused = lib.fn_opt_keras, lib.fn_opt_keras_ema
        fns[name] = lambda plain=plain, args=args: _lib.check(plain(*args, st), "optimizer pass")
        fns[name + "+ema"] = lambda fused=fused, args=args: _lib.check(fused(*args, p(shadow), 0.9999, st), "optimizer pass + ema")
        per_elem = 4.0 * (3 + 2 * len(r.slots))            # w read + written, g read, each slot read + written
        nbytes[name], nbytes[name + "+ema"] = per_elem * n + 2.0 * n_lp, (per_elem + 8.0) * n + 2.0 * n_lp
    ms = alternate(fns, warmup, windows, per_window)
    res = {"params": n, "packed": n_lp}
    for k, times in ms.items():
        t = statistics.median(times) * 1e-3
        res[k] = {"us": round(t * 1e6, 2), "bytes_per_param": round(nbytes[k] / n, 2), "tb_per_s": round(nbytes[k] / t / 1e12, 3),
                  "copy_rate_share": round(nbytes[k] / t / COPY_RATE, 3), "us_windows": [round(x * 1e3, 2) for x in times]}
    return res


def training_step(warmup, windows, per_window, batch):
    tune = tempfile.NamedTemporaryFile(suffix=".json", delete=False)      # every trainer on the same convolution tiles
    tune.close()
    os.unlink(tune.name)
    os.environ.setdefault("FACENET_TUNE_CACHE", tune.name)
    rng = np.random.default_rng(0)
    x = torch.from_numpy(rng.integers(0, 256, (batch, 160, 160, 3), dtype=np.uint8))
    y = torch.from_numpy(rng.integers(0, 10575, batch))
    params, fns, launches = None, {}, {}
    for name in OPTIMIZERS:
        net = Network(embedding_size=512, nrof_classes=10575, device="cuda:0", train_dtype=torch.bfloat16, infer_dtype=torch.float16,
                      seed=0)
        if params is None:
            params = net.export_keras_params()
        net.load_keras_params(params)
        tr = Trainer(net, batch=batch, loss="softmax", lr=1e-4, optimizer=name)
        tr.set_images(x, y)
        tr.capture()
        fns[name] = tr.step
        launches[name] = len(tr.step_ops)
    ms = alternate(fns, warmup, windows, per_window)
    adam = statistics.median(ms["ADAM"])
    return {"batch": batch, "launches": launches,
            **{k: {"ms": round(statistics.median(v), 4), "vs_adam_us": round((statistics.median(v) - adam) * 1e3, 2),
                   "windows_ms": [round(t, 4) for t in v]} for k, v in ms.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--windows", type=int, default=10)
    ap.add_argument("--per-window", type=int, default=20)
    ap.add_argument("--batch", type=int, default=90, help="images per captured softmax step")
    ap.add_argument("--skip-step", action="store_true", help="time the optimiser pass only")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    lib = _lib.load()
    out = {"kernel": {label: optimizer_pass(lib, net, a.warmup, a.windows, a.per_window) for label, net in (
        ("softmax_e512_c10575", Network(embedding_size=512, nrof_classes=10575, allocate=False)),
        ("v1_triplet_e128", Network(embedding_size=128, allocate=False)))}}
    if not a.skip_step:
        out["step"] = training_step(a.warmup, a.windows, a.per_window, a.batch)
    line = json.dumps(out)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
