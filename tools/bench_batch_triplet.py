"""What training on the whole P x K batch costs next to the mined step, on one MI355X, one job at a time.

Configurations, every one replayed from captured graphs at E = 128 (bf16 training, f16 mining forward, the tiles of the committed
tile cache; shapes it lacks are tuned into a private copy):
  mined            the step as it was: 180-image pool through the inference plan -> distances -> 30 triplets -> gather -> the
                   90-image training step (TripletMiner + Trainer: the baseline)
  batch_hard_90, batch_all_90, batch_hard_180, batch_all_180
                   one training step on the whole batch (30 x 3 or 45 x 4 images), mined inside it by fn_batch_triplet_fwd_bwd

Without --config this is the driver: it opens no GPU itself and starts every measurement as a child process of its own under its
own `timeout`, one after the other, and stops at the first child that fails.  Per configuration: a timing child (host clock around
windows of steps that end in a device synchronise, median of the windows) and, apart from it, a `rocprofv3 --kernel-trace --stats`
child whose per-kernel device times give the head's launches -- for the mined path its selection chain (l2norm_fwd,
pairwise_sqdist, select_triplets, gather_images, the triplet head).  Writes the report to --out."""
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

CONFIGS = {"mined": ("mined", 90), "batch_hard_90": ("batch_hard", 90), "batch_all_90": ("batch_all", 90),
           "batch_hard_180": ("batch_hard", 180), "batch_all_180": ("batch_all", 180)}
POOL, E = 180, 128
# kernels of the selection chain and of the two heads, by the names the trace shows (fill_words_kernel also zeroes other small words)
CHAIN = ("l2norm_fwd_kernel", "l2norm_bwd_kernel", "pairwise_kernel", "select_pairs_kernel", "select_negatives_kernel", "select_rank_kernel",
         "gather_images_kernel", "triplet_loss_kernel", "loss_finish_kernel", "batch_triplet_mine_kernel", "batch_triplet_finish_kernel",
         "batch_triplet_gather_kernel", "fill_words_kernel")


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
    from facenet_amd.schedule import make_events
    from facenet_amd.train import GraphRunner, Trainer, TripletMiner
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    strategy, B = CONFIGS[config]
    dev = torch.device("cuda", 0)
    net = Network(embedding_size=E, device=str(dev), train_dtype=torch.bfloat16, infer_dtype=torch.float16, seed=0)
    g = torch.Generator(device=dev).manual_seed(1234)
    n_in = POOL if strategy == "mined" else B
    pools = [torch.randint(0, 256, (n_in, 160, 160, 3), dtype=torch.uint8, device=dev, generator=g) for _ in range(4)]
    K = 4 if n_in % 4 == 0 else 3            # 180 = 45 x 4 (the pool of the mined step), 90 = 30 x 3
    labels = np.repeat(np.arange(n_in // K), K)
    if strategy == "mined":
        trainer = Trainer(net, batch=B, loss="triplet", alpha=0.2, lr=0.05)
        miner = TripletMiner(net, POOL, labels, B // 3, alpha=0.2, seed=0)
        miner.build(trainer.plan.images)
        miner.plan.images.copy_(pools[0])
        miner.run()
        trainer.step_eager()
        torch.cuda.synchronize()
        events = make_events(miner.sched)
        mine_graph = GraphRunner(dev).capture(lambda: miner.run(events))
        trainer.capture()

        def step(i):
            miner.plan.images.copy_(pools[i % len(pools)])
            mine_graph.replay()
            trainer.step()
        chain = ("l2norm_fwd", "pairwise_sqdist", "select_triplets", "gather_images")
        head = [op.name for op in miner.ops if op.name in chain] + [op.name for op in trainer.loss_ops]
        embedded = POOL + B
    else:
        trainer = Trainer(net, batch=B, loss="triplet", alpha=0.2, lr=0.05, triplet_strategy=strategy)
        trainer.set_images(pools[0], labels)
        trainer.step_eager()
        torch.cuda.synchronize()
        trainer.capture()

        def step(i):
            trainer.plan.images.copy_(pools[i % len(pools)])
            trainer.step()
        head = [op.name for op in trainer.loss_ops]
        embedded = B
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
    out = {"config": config, "batch": B, "ms_per_step": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
           "windows": windows, "steps_per_window": steps, "images_embedded_per_s": round(1e3 * embedded / med, 1),
           "images_trained_per_s": round(1e3 * B / med, 1), "loss": round(trainer.loss_value(), 5), "head_launches": head,
           "steps_run": 2 + warmup + windows * steps}      # + the eager step before the capture and capture()'s own warm-up step
    if strategy != "mined":
        out["triplet_stats"] = trainer.triplet_stats()
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
        for k in CHAIN:
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
    ap.add_argument("--out", default=str(ROOT / "profiles" / "batch_triplet_bench.txt"))
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
    lines = ["tools/bench_batch_triplet.py on one MI355X: v1, E 128, bf16 training; every step replayed from captured graphs; synthetic uint8",
             f"images resident on the device.  Per configuration two processes (alternating rounds), each {a.windows} windows of {a.steps} steps after",
             f"{a.warmup} warm-up steps; host clock around a window that ends in a device synchronise.  ms = median of a process's windows",
             "[min, max over its windows].  embedded = images through a forward per second (mined: 180 pool + 90 batch); trained = images",
             "that receive a gradient per second.", "",
             f"{'configuration':<16}{'batch':>6}{'ms / step (round 1)':>30}{'ms / step (round 2)':>30}{'embedded img/s':>16}{'trained img/s':>15}{'active':>9}"]
    for c, rs in runs.items():
        best = min(rs, key=lambda r: r["ms_per_step"])
        cells = [f"{r['ms_per_step']:.3f} [{r['ms_min']:.3f}, {r['ms_max']:.3f}]" for r in rs]
        act = f"{best['triplet_stats']['active_fraction']:.3f}" if "triplet_stats" in best else "-"
        lines.append(f"{c:<16}{best['batch']:>6}{cells[0]:>30}{cells[1]:>30}{best['images_embedded_per_s']:>16.1f}{best['images_trained_per_s']:>15.1f}{act:>9}")
    lines += ["", "(img/s from the faster round of each configuration.)"]
    if not a.no_kernel_stats:
        scratch = tempfile.mkdtemp(prefix="batch_triplet_prof_")
        lines += ["", "Device time of the head's kernels, rocprofv3 --kernel-trace --stats, one profiler run per configuration (apart from the",
                  "timings above): per launch = the kernel's total over the run / its calls; launches per step = calls / the steps the run",
                  "made (2 eager + warm-up + timed), rounded; us per step = their product.  A traced duration carries the dispatch floor of",
                  "about 3 us per launch.", ""]
        for c in ("mined", "batch_hard_90", "batch_all_90", "batch_hard_180", "batch_all_180"):
            stats, total, steps = kernel_stats(c, a.limit, scratch)
            lines.append(f"{c}: {steps} steps, all kernels {total / steps / 1e3:.3f} ms of device time per step; head launches: {', '.join(runs[c][0]['head_launches'])}")
            chain = 0.0
            for k in CHAIN:
                if k in stats:
                    calls, dur = stats[k]
                    per_step = max(1, round(calls / steps))
                    chain += per_step * dur / calls
                    lines.append(f"    {k:<32}{calls:>6} calls{dur / calls:>10.2f} us per launch{per_step:>4} per step{per_step * dur / calls:>10.2f} us per step")
            lines.append(f"    {'sum':<32}{'':>12}{'':>24}{'':>13}{chain:>10.2f} us per step")
        shutil.rmtree(scratch, ignore_errors=True)
    lines += ["", "raw: " + json.dumps(runs)]
    Path(a.out).write_text("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
