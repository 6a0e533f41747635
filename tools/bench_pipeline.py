"""Loader throughput on the GPU box: synthetic 250x250 JPEG files (the VGGFace2/CASIA crops the reference trains on are
about that size) -> thread-pool decode -> pinned staging -> H2D -> fn_crop_or_pad_u8.  Prints images/s for several worker
counts, and the device-only rate of the crop kernel.

``--resident [--per-class K]`` runs the resident leg instead, on the same kind of set with K files per
class: end-to-end images/s of BatchPipeline (8 worker processes) against ResidentPipeline, alternated, at batch 100 and 180 with
the augmentation keys off and on; device time per launch of fn_resident_batch_u8 against fn_augment_u8 on the same images (HIP
events, interleaved rounds); and the seconds to build a pack and to load it into device memory.  ``--resident-train`` times the
batch-hard train_tripletloss app fed both ways.  One JSON line per figure."""
import json, random, statistics, sys, tempfile, time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from facenet_amd import dataset
from facenet_amd.config import Config


def write_jpegs(root, per_class=25):
    from PIL import Image
    rng = np.random.default_rng(0)
    for c in range(40):
        (root / f"c{c:02d}").mkdir()
        for i in range(per_class):
            base = rng.integers(0, 256, (32, 32, 3), dtype=np.uint8)
            img = np.asarray(Image.fromarray(base).resize((250, 250), Image.BILINEAR))
            Image.fromarray(img).save(root / f"c{c:02d}" / f"{i:03d}.jpg", quality=90)


def pipeline_rate(pipe, images):
    """images/s of a repeating pipeline over at least `images` images after the first batch (worker start-up, first launches)."""
    n, t0 = 0, None
    for x, _ in pipe:
        if t0 is None:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            continue
        n += x.shape[0]
        if n >= images:
            break
    torch.cuda.synchronize()
    rate = n / (time.perf_counter() - t0)
    pipe.close()
    return rate


def launch_times(store, arrays_of, size=160, n=100, reps=200, rounds=7):
    """Device microseconds per launch, HIP events around `reps` launches, the two entries interleaved over `rounds` rounds."""
    from facenet_amd import _lib
    lib = _lib.load()
    st = torch.cuda.current_stream()
    rows = np.random.default_rng(1).permutation(store.nrof_images)[:n].astype(np.int32)
    arrays = [arrays_of(int(r)) for r in rows]
    hw = np.array([a.shape[:2] for a in arrays], np.int32)
    off = np.concatenate([[0], np.cumsum([a.size for a in arrays])[:-1]]).astype(np.int64)
    d_src = torch.from_numpy(np.concatenate([a.reshape(-1) for a in arrays])).cuda()
    d_off, d_hw, d_rows = torch.from_numpy(off).cuda(), torch.from_numpy(hw).cuda(), torch.from_numpy(rows).cuda()
    d_iota = torch.arange(n, dtype=torch.int32, device="cuda")
    out = torch.empty(n, size, size, 3, dtype=torch.uint8, device="cuda")
    for path, keys in (("copy", (False, False, False)), ("rotated", (True, True, True))):
        draws = dataset.Augmentation(*keys, seed=1).draw(n)
        prm = torch.from_numpy(dataset.augment_params(draws, hw, size).view(np.uint8)).cuda()
        launches = {
            "fn_augment_u8": lambda: lib.fn_augment_u8(d_src.data_ptr(), d_off.data_ptr(), d_hw.data_ptr(), prm.data_ptr(), out.data_ptr(), n,
                                                       size, st.cuda_stream),
            "fn_resident_batch_u8": lambda: lib.fn_resident_batch_u8(store.pool.data_ptr(), store.offsets.data_ptr(), store.hw.data_ptr(),
                                                                     store.nrof_images, d_rows.data_ptr(), prm.data_ptr(), out.data_ptr(), n,
                                                                     size, st.cuda_stream),
            # the same entry on fn_augment_u8's own buffer and tables with rows 0 .. n-1: the row indirection without the large pool
            "fn_resident_batch_u8, batch-local pool": lambda: lib.fn_resident_batch_u8(d_src.data_ptr(), d_off.data_ptr(), d_hw.data_ptr(), n,
                                                                                       d_iota.data_ptr(), prm.data_ptr(), out.data_ptr(), n,
                                                                                       size, st.cuda_stream),
        }
        check = {}
        for name, launch in launches.items():
            for _ in range(20):
                _lib.check(launch())
            check[name] = out.clone()
        assert all(torch.equal(v, check["fn_augment_u8"]) for v in check.values()), "the entries disagree"
        us = {name: [] for name in launches}
        for _ in range(rounds):
            for name, launch in launches.items():
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(reps):
                    launch()
                t1.record()
                t1.synchronize()
                us[name].append(t0.elapsed_time(t1) * 1e3 / reps)
        for name, v in us.items():
            print(json.dumps({"launch": name, "path": path, "batch": n, "size": size, "us_median": round(statistics.median(v), 2),
                              "us_min": round(min(v), 2), "us_max": round(max(v), 2), "rounds": rounds, "reps": reps}), flush=True)


def resident_leg(per_class):
    from facenet_amd import resident
    with tempfile.TemporaryDirectory() as d:
        root = Path(d) / "data"
        root.mkdir()
        t0 = time.perf_counter()
        write_jpegs(root, per_class)
        db = dataset.Database(Config({"path": str(root)}))
        print(json.dumps({"set": f"40 classes x {per_class} JPEG 250x250 (quality 90)", "images": db.nrof_images,
                          "written_in_s": round(time.perf_counter() - t0, 1)}), flush=True)
        loader = dataset.ImageLoader(Config({"size": 160}))
        # 3. build and load times
        t0 = time.perf_counter()
        pack = resident.build_pack(db, Path(d) / "pack", workers=8)
        build = time.perf_counter() - t0
        print(json.dumps({"pack_build_s": round(build, 2), "images": pack.nrof_images, "bytes": pack.nbytes, "decode_threads": 8,
                          "images_per_s": round(pack.nrof_images / build)}), flush=True)
        for k in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            store = resident.ResidentDataset.from_database(db, cache=Path(d) / "pack")
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            print(json.dumps({"pack_load_s": round(dt, 3), "run": k, "bytes": store.nbytes, "GB_per_s": round(store.nbytes / dt / 1e9, 2),
                              "upload_only_s": round(store.info["load_seconds"], 3), "cache": store.info["cache"],
                              "note": "validity check (stat of every file) + memmap read from the page cache + pinned staging + H2D"}),
                  flush=True)
        # 1. end to end, the two pipelines alternated, two runs each
        on = dict(random_crop=True, random_flip=True, random_rotate=True)
        for batch in (100, 180):
            for augmented in (False, True):
                for run in range(2):
                    for name in ("BatchPipeline processes 8", "ResidentPipeline"):
                        aug = dataset.Augmentation(**on, seed=0) if augmented else None
                        kw = dict(resident=store) if name == "ResidentPipeline" else dict(workers=8, prefetch=4, processes=True)
                        pipe = db.tf_dataset_api(loader, batch_size=batch, buffer_size=10, repeat=True, augment=aug, **kw)
                        rate = pipeline_rate(pipe, 400000 if name == "ResidentPipeline" else 20000)
                        print(json.dumps({"pipeline": name, "batch": batch, "augment": augmented, "run": run, "images_per_s": round(rate)}),
                              flush=True)
        # 2. device time per launch
        for n in (100, 180):
            launch_times(store, store.image, n=n)


def train_leg(per_class, steps=300):
    """Optional: the batch-hard train_tripletloss app (20 x 5 images per step, all augmentation keys on) fed from the files and
    from the store, alternated, two runs each; the app's own epoch lines (the second epoch is the steady one)."""
    from facenet_amd.apps import train_tripletloss as tt
    from facenet_amd.config import load_config
    with tempfile.TemporaryDirectory() as d:
        root = Path(d) / "data"
        root.mkdir()
        write_jpegs(root, per_class)
        for run in range(2):
            for name, keys in (("files, 8 worker processes", {}), ("resident", {"resident": True})):
                cfg = load_config(None, {"seed": 0, "image": {"size": 160, "normalization": 0, "random_crop": True, "random_flip": True,
                                                              "random_rotate": True},
                                         "dataset": {"path": str(root), **keys}, "loss": {"triplet_strategy": "batch_hard"},
                                         "train": {"epoch": {"nrof_epochs": 2, "size": steps}, "learning_rate": {"schedule": [[2, 0.05]]}}})
                logs = []
                random.seed(0)                            # the sampler draws from `random`: both feeds train on the same batches
                pipe = tt.dataset_pools(cfg, log=logs.append, workers=8, prefetch=4)
                tt.train_tripletloss(cfg, people_per_batch=cfg.nrof_classes_per_batch, images_per_person=cfg.nrof_examples_per_class,
                                     pools=pipe, log=logs.append)
                pipe.close()
                for line in logs:
                    if line.startswith(("epoch", "resident")):
                        print(json.dumps({"train_tripletloss batch_hard": name, "run": run, "steps_per_epoch": steps, "log": line}), flush=True)


def main():
    per_class = int(sys.argv[sys.argv.index("--per-class") + 1]) if "--per-class" in sys.argv else 25
    if "--resident" in sys.argv or "--resident-train" in sys.argv:
        assert torch.cuda.is_available(), "the resident leg needs the MI355X"
        if "--resident" in sys.argv:
            resident_leg(per_class)
        if "--resident-train" in sys.argv:
            train_leg(per_class)
        return
    with tempfile.TemporaryDirectory() as d:
        root = Path(d)
        write_jpegs(root)
        db = dataset.Database(Config({"path": str(root)}))
        loader = dataset.ImageLoader(Config({"size": 160}))
        for workers, procs in ((1, False), (4, False), (4, True), (8, True), (16, True)):
            pipe = db.tf_dataset_api(loader, batch_size=100, buffer_size=10, repeat=True, workers=workers, prefetch=4, processes=procs)
            n, t0 = 0, None
            for images, labels in pipe:
                if t0 is None:
                    t0 = time.perf_counter()          # first batch = warm-up
                    continue
                n += images.shape[0]
                if n >= 6000:
                    break
            torch.cuda.synchronize()
            pipe.close()
            print(f"{'processes' if procs else 'threads  '} {workers:2d}: {n / (time.perf_counter() - t0):9.0f} images/s (decode + pack + H2D + crop)", flush=True)
        arrays = [loader.decode(f) for f in db.files[:100]]
        out = dataset.crop_or_pad_batch(arrays, 160)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(20):
            out = dataset.crop_or_pad_batch(arrays, 160, staging=getattr(out, "_staging", None))
        torch.cuda.synchronize()
        print(f"pack + H2D + crop only: {2000 / (time.perf_counter() - t0):9.0f} images/s", flush=True)


if __name__ == "__main__":
    main()
