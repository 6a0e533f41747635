"""Times the landmark alignment (fn_face_align_u8) against the box crop it can replace
(fn_face_crop_resize_u8, section 17): F = 1, 16 and 256 faces at S = 160 out of a resident 1280 x 720 frame, at about 1, 2 and 4
source pixels per output pixel (n = 1, 2, 4 sub-samples per axis for the alignment; windows of 161, 321 and 641 pixels for the
Lanczos crop).  Each call is the whole entry point: the copy of its host tables plus its launches.

Both paths alternate in one process; every sample is a device-event window around enough back-to-back calls to last about 20 ms,
after a warm-up of both; the figure is the median of --reps samples.  The first face of every shape is compared with
tests/align_oracle.py bit for bit.  Prints a table, optionally writes it to --out, and ends with one JSON line.

    python tools/bench_align.py [--reps 7] [--out profiles/align_bench.txt]"""
import argparse
import ctypes
import json
import math
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from facenet_amd import _lib
from tests import align_oracle as ao

H, W, S = 720, 1280, 160
HBM_PEAK = 8.0e12

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--out", type=Path, default=None)
args = ap.parse_args()
assert torch.cuda.is_available(), "bench_align needs the MI355X"
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
    """paths: name -> callable.  Warm up, size the windows, then alternate the paths `reps` times -> name -> seconds per call."""
    inner = {}
    for name, fn in paths.items():
        window(fn, 3)
        inner[name] = max(1, min(2000, int(0.02 / max(window(fn, 3), 1e-6))))
    samples = {name: [] for name in paths}
    for _ in range(reps):
        for name, fn in paths.items():
            samples[name].append(window(fn, inner[name]))
    return {name: np.array(v) for name, v in samples.items()}, inner


rng = np.random.default_rng(0)
base = rng.integers(0, 256, (H // 8, W // 8, 3), dtype=np.uint8)
frame_host = np.clip(np.kron(base, np.ones((8, 8, 1), np.uint8)).astype(np.int32) + rng.integers(-12, 13, (H, W, 3)), 0, 255).astype(np.uint8)
frame = torch.from_numpy(frame_host).to(dev)
lines, results = [], []


def say(text):
    print(text, flush=True)
    lines.append(text)


say(f"fn_face_align_u8 against fn_face_crop_resize_u8, {torch.cuda.get_device_name(0)}; {W}x{H} frame, S = {S}; us per call, median (min .. max) of "
    f"{args.reps} device-event windows of about 20 ms, the two paths alternating")
say(f"{'F':>4} {'sigma':>5} {'n':>2} | {'align us':>24} | {'box crop us':>24} | {'align/crop':>10} | {'align GB/s':>10} | bytes equal the oracle")
for F in (1, 16, 256):
    for sigma in (1.0, 2.0, 4.0):
        extent = int(round(sigma * S)) + 1             # + 1: a window of exactly S pixels is a plain copy for the crop, not a resampling
        cx, cy = rng.uniform(extent / 2, W - extent / 2, F), rng.uniform(extent / 2, H - extent / 2, F)
        inverse = np.ascontiguousarray([ao.inverse_of(sigma, math.radians(a), (x, y), S) for a, x, y in zip(rng.uniform(-30, 30, F), cx, cy)])
        n = ao.samples_of(sigma)
        samples = np.full(F, n, np.int32)
        windows = np.ascontiguousarray(np.stack([cx - extent / 2, cy - extent / 2, cx - extent / 2 + extent, cy - extent / 2 + extent], axis=1).astype(np.int32))
        windows[:, 2], windows[:, 3] = windows[:, 0] + extent, windows[:, 1] + extent
        nbytes, words = ctypes.c_longlong(0), ctypes.c_longlong(0)
        _lib.check(lib.fn_face_align_workspace(F, ctypes.byref(nbytes)))
        _lib.check(lib.fn_face_crop_workspace(windows.ctypes.data, F, S, ctypes.byref(words)))
        ws_align = torch.empty(nbytes.value // 8, dtype=torch.int64, device=dev)
        ws_crop = torch.empty(words.value, dtype=torch.int32, device=dev)
        out_align = torch.empty(F, S, S, 3, dtype=torch.uint8, device=dev)
        out_crop = torch.empty(F, S, S, 3, dtype=torch.uint8, device=dev)

        def align():
            _lib.check(lib.fn_face_align_u8(frame.data_ptr(), H, W, inverse.ctypes.data, samples.ctypes.data, F, S, out_align.data_ptr(),
                                            ws_align.data_ptr(), nbytes.value, stream()))

        def crop():
            _lib.check(lib.fn_face_crop_resize_u8(frame.data_ptr(), H, W, windows.ctypes.data, F, S, 0, 0, S, out_crop.data_ptr(), ws_crop.data_ptr(),
                                                  words.value, stream()))
        t, inner = bench({"align": align, "crop": crop}, args.reps)
        same = bool(np.array_equal(out_align[0].cpu().numpy(), ao.warp(frame_host, inverse[0], n, S)))
        us = {k: (float(np.median(v)) * 1e6, float(v.min()) * 1e6, float(v.max()) * 1e6) for k, v in t.items()}
        moved = F * S * S * 3 + F * (sigma * S) ** 2 * 3                     # written + the footprint read once
        row = {"F": F, "sigma": sigma, "n": n, "align_us": [round(v, 2) for v in us["align"]], "crop_us": [round(v, 2) for v in us["crop"]],
               "ratio": round(us["align"][0] / us["crop"][0], 3), "align_GBps": round(moved / us["align"][0] / 1e3, 1),
               "hbm_floor_us": round(moved / HBM_PEAK * 1e6, 3), "calls_per_window": inner, "equals_oracle": same}
        results.append(row)
        fmt = lambda v: f"{v[0]:9.2f} ({v[1]:.2f} .. {v[2]:.2f})"
        say(f"{F:>4} {sigma:>5} {n:>2} | {fmt(us['align']):>24} | {fmt(us['crop']):>24} | {row['ratio']:>10} | {row['align_GBps']:>10} | {same}")
if args.out is not None:
    args.out.parent.mkdir(parents=True, exist_ok=True)
    args.out.write_text("\n".join(lines) + "\n")
ok = all(r["equals_oracle"] for r in results)
print(json.dumps({"bench": "align", "device": torch.cuda.get_device_name(0), "equals_oracle_everywhere": ok, "shapes": results}))
sys.exit(0 if ok else 1)
