"""fn_augment_u8 against fn_crop_or_pad_u8 on the MI355X: device time per batch of 100 ragged-packed
182x182 and 250x250 sources -> 160x160, from HIP events after warm-up, for every key combination; the share of the HBM bound
with bytes counted from shapes (the least any of them moves: the S x S window read once, the output written once, and
the per-image metadata); and the end-to-end pipeline rate with 8
worker processes, augmentation on and off.  Prints one JSON line per figure."""
import itertools
import json
import sys
import tempfile
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from facenet_amd import _lib, dataset
from facenet_amd.config import Config

HBM_BYTES_PER_S = 8.0e12        # MI355X HBM3E peak (spec)
N, S, REPS = 100, 160, 200


def device_times(src_hw):
    lib = _lib.load()
    rng = np.random.default_rng(0)
    arrays = [rng.integers(0, 256, (src_hw, src_hw, 3), dtype=np.uint8) for _ in range(N)]
    st = torch.cuda.current_stream()
    off = torch.arange(N, dtype=torch.int64, device="cuda") * (src_hw * src_hw * 3)
    hw = torch.full((N, 2), src_hw, dtype=torch.int32, device="cuda")
    src = torch.from_numpy(np.stack(arrays)).cuda().view(-1)
    out = torch.empty(N, S, S, 3, dtype=torch.uint8, device="cuda")
    nbytes = 2 * N * S * S * 3 + N * 16
    launches = {"crop_or_pad": lambda: lib.fn_crop_or_pad_u8(src.data_ptr(), off.data_ptr(), hw.data_ptr(), out.data_ptr(), N, S, st.cuda_stream)}
    for crop, flip, rotate in itertools.product((False, True), repeat=3):
        draws = dataset.Augmentation(random_crop=crop, random_flip=flip, random_rotate=rotate, seed=1).draw(N)
        prm = torch.from_numpy(dataset.augment_params(draws, [(src_hw, src_hw)] * N, S).view(np.uint8)).cuda()
        name = "augment[" + ",".join(k for k, on in zip(("crop", "flip", "rotate"), (crop, flip, rotate)) if on) + "]"
        launches[name] = (lambda p: lambda: lib.fn_augment_u8(src.data_ptr(), off.data_ptr(), hw.data_ptr(), p.data_ptr(), out.data_ptr(), N, S,
                                                              st.cuda_stream))(prm)
    for name, launch in launches.items():
        for _ in range(20):
            _lib.check(launch())
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(REPS):
            launch()
        t1.record()
        t1.synchronize()
        us = t0.elapsed_time(t1) * 1e3 / REPS
        b = nbytes + (N * 20 if name.startswith("augment") else 0)
        print(json.dumps({"kernel": name, "src": f"{src_hw}x{src_hw}", "batch": N, "size": S, "us_per_batch": round(us, 2),
                          "bytes": b, "hbm_bound_us": round(b / HBM_BYTES_PER_S * 1e6, 2),
                          "share_of_hbm_bound": round(b / HBM_BYTES_PER_S * 1e6 / us, 3)}), flush=True)


def pipeline_rates():
    from PIL import Image
    rng = np.random.default_rng(0)
    with tempfile.TemporaryDirectory() as d:
        root = Path(d)
        for c in range(40):
            (root / f"c{c:02d}").mkdir()
            for i in range(25):
                base = rng.integers(0, 256, (32, 32, 3), dtype=np.uint8)
                img = np.asarray(Image.fromarray(base).resize((250, 250), Image.BILINEAR))
                Image.fromarray(img).save(root / f"c{c:02d}" / f"{i:03d}.jpg", quality=90)
        db = dataset.Database(Config({"path": str(root)}))
        loader = dataset.ImageLoader(Config({"size": S}))
        for aug in (None, dataset.Augmentation(random_crop=True, random_flip=True, random_rotate=True, seed=0)) * 2:
            pipe = db.tf_dataset_api(loader, batch_size=N, buffer_size=10, repeat=True, workers=8, prefetch=4, processes=True, augment=aug)
            n, t0 = 0, None
            for images, _ in pipe:
                if t0 is None:
                    t0 = time.perf_counter()          # first batch = warm-up (worker start-up)
                    continue
                n += images.shape[0]
                if n >= 6000:
                    break
            torch.cuda.synchronize()
            rate = n / (time.perf_counter() - t0)
            pipe.close()
            print(json.dumps({"pipeline": "processes 8", "augment": aug is not None, "images_per_s": round(rate)}), flush=True)


if __name__ == "__main__":
    assert torch.cuda.is_available(), "bench_augment needs the MI355X"
    for src_hw in (182, 250):
        device_times(src_hw)
    pipeline_rates()
