"""What a cross-batch memory adds to the batch-hard step, on one MI355X, one job at a time.

Configurations, every one the v1 batch-hard step on 45 x 4 = 180 images at E = 128 (bf16 training, the tiles of the committed tile
cache; shapes it lacks are tuned into a private copy), replayed from captured graphs:
  off              no memory: the step of section 31 (the baseline of the same job)
  m4096, m16384, m65536
                   the same step mined over the batch and a memory of that many rows, full from the first replayed step on

Without --config this is the driver: it opens no GPU itself and starts every measurement as a child process of its own under its
own `timeout`, one after the other, and stops at the first child that fails.  Per configuration: two timing children in alternating
rounds (host clock around windows of steps that end in a device synchronise, median of the windows) and, apart from them, one
`rocprofv3 --kernel-trace --stats` child whose per-kernel device times give the head's launches.  Writes the report to --out."""
import argparse
import glob
import json
import os
import shutil
import sqlite3
import statistics
import subprocess
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

CONFIGS = {"off": 0, "m4096": 4096, "m16384": 16384, "m65536": 65536}
B, K, E, IDENTITIES = 180, 4, 128, 2000
# the head's kernels by the names the trace shows (fill_words_kernel also zeroes other small words; pairwise_kernel runs twice with a memory)
HEAD = ("l2norm_fwd_kernel", "l2norm_bwd_kernel", "pairwise_kernel", "batch_triplet_mine_kernel", "batch_triplet_finish_kernel",
        "batch_triplet_gather_kernel", "xbm_triplet_mine_kernel", "xbm_triplet_gather_kernel", "xbm_enqueue_copy_kernel",
        "xbm_enqueue_advance_kernel", "fill_words_kernel")


def tile_cache():
    """A private copy of the committed tile choices, as bench.py takes them."""
    if "FACENET_TUNE_CACHE" in os.environ:
        return
    found = sorted(glob.glob(str(ROOT / "profiles" / "r[0-9][0-9]_tile_cache.json")))
    if found:
        fd, cache = tempfile.mkstemp(prefix="facenet_tiles_", suffix=".json")
        os.close(fd)
        shutil.copyfile(found[-1], cache)
        os.environ["FACENET_TUNE_CACHE"] = cache


def measure(config, steps, warmup, windows):
    """One configuration in this process -> a JSON line."""
    tile_cache()
    import numpy as np
    import torch
    from facenet_amd.engine import Network
    from facenet_amd.train import Trainer
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    M = CONFIGS[config]
    dev = torch.device("cuda", 0)
    net = Network(embedding_size=E, device=str(dev), train_dtype=torch.bfloat16, infer_dtype=torch.float16, seed=0)
    g = torch.Generator(device=dev).manual_seed(1234)
    pools = [torch.randint(0, 256, (B, 160, 160, 3), dtype=torch.uint8, device=dev, generator=g) for _ in range(4)]
    rng = np.random.default_rng(0)
    # 45 of 2000 identities per step: like a large training set, an identity of the batch has a handful of rows in the memory
    label_sets = [torch.from_numpy(np.repeat(rng.choice(IDENTITIES, B // K, replace=False), K).astype(np.int32)).to(dev) for _ in range(4)]
    trainer = Trainer(net, batch=B, loss="triplet", alpha=0.2, lr=0.05, triplet_strategy="batch_hard", memory_size=M)
    trainer.set_images(pools[0], label_sets[0].cpu())
    trainer.step_eager()
    torch.cuda.synchronize()
    trainer.capture()

    def step(i):
        trainer.plan.images.copy_(pools[i % len(pools)])
        trainer.labels.copy_(label_sets[i % len(label_sets)])
        trainer.step()
    if M:
        # the ring is filled here, not by M / 180 steps, so that every step of the run -- a profiler's run included -- mines over all
        # M rows: random unit rows under random identities, which the steps then overwrite 180 at a time
        rows = torch.randn(M, E, device=dev, generator=g)
        trainer.mem_emb.copy_(rows / rows.norm(dim=1, keepdim=True))
        trainer.mem_labels.copy_(torch.from_numpy(rng.integers(0, IDENTITIES, M).astype(np.int32)).to(dev))
        trainer.mem_state.copy_(torch.tensor([0, M, 1, 0], dtype=torch.int32))
    for i in range(warmup):
        step(i)
    torch.cuda.synchronize()
    ms = []
    for _ in range(windows):
        t0 = time.perf_counter()
        for i in range(steps):
            step(i)
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0) / steps)
    med = statistics.median(ms)
    out = {"config": config, "memory": M, "batch": B, "ms_per_step": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
           "windows": windows, "steps_per_window": steps, "images_trained_per_s": round(1e3 * B / med, 1), "loss": round(trainer.loss_value(), 5),
           "head_launches": [op.name for op in trainer.loss_ops], "triplet_stats": trainer.triplet_stats(),
           "steps_run": 2 + warmup + windows * steps}      # + the eager step before the capture and capture()'s own warm-up step
    print(json.dumps(out), flush=True)


def child(argv, limit, env=None):
    """One child under its own time limit -> its stdout; a failure ends the driver (nothing more is started on the GPU)."""
    cmd = ["timeout", "-k", "10", str(limit)] + argv
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=str(ROOT), env=env)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit(f"{' '.join(cmd)} ended with status {r.returncode}: stopping")
    return r.stdout


def last_json(text):
    return json.loads([ln for ln in text.splitlines() if ln.startswith("{")][-1])


def kernel_stats(config, limit, scratch):
    """Per-kernel device time of one configuration from a profiler run of its own: {kernel: (calls, total us)}, the device time
    of all kernels and the steps the run made."""
    d = os.path.join(scratch, "prof_" + config)
    text = child(["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "st", "--", sys.executable, str(Path(__file__).resolve()),
                  "--config", config, "--steps", "10", "--warmup", "2", "--windows", "2"], limit)
    run = last_json(text)
    dbs = glob.glob(os.path.join(d, "**", "st_results.db"), recursive=True)
    assert dbs, f"no rocpd database under {d}"
    rows = sqlite3.connect(dbs[0]).execute("select name, total_calls, total_duration from top_kernels").fetchall()
    total = sum(r[2] for r in rows)
    stats = {}
    for name, calls, dur in rows:
        for k in HEAD:
            if k in name:                    # (the database holds mangled names)
                c, t = stats.get(k, (0, 0.0))
                stats[k] = (c + calls, t + dur)
    return stats, total, run["steps_run"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=sorted(CONFIGS), help="measure this configuration in this process (what the driver starts)")
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--limit", type=int, default=240, help="seconds each child may take")
    ap.add_argument("--no-kernel-stats", action="store_true")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "xbm_bench.txt"))
    a = ap.parse_args()
    if a.config:
        return measure(a.config, a.steps, a.warmup, a.windows)
    tile_cache()                             # one private copy for all children: a shape it lacks is tuned by the first child that meets it
    me = [sys.executable, str(Path(__file__).resolve())]
    runs = {}
    for rnd in range(2):                     # two alternating rounds: the spread between them is the noise of the shared host
        for c in CONFIGS:
            runs.setdefault(c, []).append(last_json(child(me + ["--config", c, "--steps", str(a.steps), "--warmup", str(a.warmup),
                                                                "--windows", str(a.windows)], a.limit)))
    base = min(r["ms_per_step"] for r in runs["off"])
    lines = ["tools/bench_xbm.py on one MI355X: v1, E 128, bf16 training, batch hard on 45 x 4 = 180 images drawn from 2000 identities; every step",
             "replayed from captured graphs; synthetic uint8 images resident on the device; the memory is filled with random unit rows before the",
             f"first replay.  Per configuration two processes (alternating rounds), each {a.windows} windows of {a.steps} steps after {a.warmup} warm-up steps; host clock around a window that",
             "ends in a device synchronise.  ms = median of a process's windows [min, max over its windows].  added = the faster round minus the",
             "faster round of `off` in the same job.  active and mem neg (the share of anchors whose nearest negative was a memory slot, last step)",
             "describe that synthetic ring next to an untrained network's embeddings, not a training run.", "",
             f"{'configuration':<14}{'memory':>8}{'ms / step (round 1)':>30}{'ms / step (round 2)':>30}{'added ms':>10}{'trained img/s':>15}{'active':>8}{'mem neg':>9}"]
    for c, rs in runs.items():
        best = min(rs, key=lambda r: r["ms_per_step"])
        cells = [f"{r['ms_per_step']:.3f} [{r['ms_min']:.3f}, {r['ms_max']:.3f}]" for r in rs]
        st = best["triplet_stats"]
        neg = f"{st['memory_negatives'] / max(st['anchors'], 1):.3f}" if "memory_negatives" in st else "-"
        lines.append(f"{c:<14}{best['memory']:>8}{cells[0]:>30}{cells[1]:>30}{best['ms_per_step'] - base:>10.3f}{best['images_trained_per_s']:>15.1f}"
                     f"{st['active_fraction']:>8.3f}{neg:>9}")
    if not a.no_kernel_stats:
        scratch = tempfile.mkdtemp(prefix="xbm_prof_")
        lines += ["", "Device time of the head's kernels, rocprofv3 --kernel-trace --stats, one profiler run per configuration (apart from the",
                  "timings above): per launch = the kernel's total over the run / its calls; launches per step = calls / the steps the run",
                  "made, rounded; us per step = their product.  pairwise_kernel runs twice per step with a memory ([180,180] and [180,M]): its",
                  "per-launch figure is the mean of the two, its per-step figure their sum.  A traced duration carries the dispatch floor of",
                  "about 3 us per launch.", ""]
        sums = {}
        for c in CONFIGS:
            stats, total, steps = kernel_stats(c, a.limit, scratch)
            lines.append(f"{c}: {steps} steps, all kernels {total / steps / 1e3:.3f} ms of device time per step; head launches: {', '.join(runs[c][0]['head_launches'])}")
            chain = 0.0
            for k in HEAD:
                if k in stats:
                    calls, dur = stats[k]
                    per_step = max(1, round(calls / steps))
                    chain += per_step * dur / calls
                    lines.append(f"    {k:<32}{calls:>6} calls{dur / calls:>10.2f} us per launch{per_step:>4} per step{per_step * dur / calls:>10.2f} us per step")
            sums[c] = chain
            lines.append(f"    {'sum':<32}{'':>12}{'':>24}{'':>13}{chain:>10.2f} us per step   (+{chain - sums['off']:.2f} us over off)")
        shutil.rmtree(scratch, ignore_errors=True)
    lines += ["", "raw: " + json.dumps(runs)]
    Path(a.out).write_text("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
