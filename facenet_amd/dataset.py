"""Input pipeline on the left edge of the step (reference: facenet/dataset.py, facenet/facenet.py:45-54).

Directory-per-class listing (`ImageClass`, `Database`), the shuffled batch iterator (`tf_dataset_api`) and the P x K
identity sampler (`pipeline_with_equal_batches`) keep the reference's names, attributes and errors.  What changes is
where the pixels are handled: a thread pool decodes files to ragged HWC uint8 arrays, a batch is packed back to back
into pinned host memory, copied on a side stream and centre-cropped / zero-padded on the GPU
(`fn_crop_or_pad_u8` = tf.image.resize_with_crop_or_pad) -- or, for training with an `Augmentation`, randomly rotated,
cropped and flipped in the same single launch (`fn_augment_u8`) -- so what reaches the step is the
uint8 NHWC batch its first kernel (`fn_image_normalize`) reads.  Batches are prefetched `prefetch` deep; the consumer's stream waits on an event.
With a `resident` store (facenet_amd.resident) the decoded set already lives on the device and
`ResidentPipeline` builds the same batches from it by row number, with no decode and no pixel copy per batch.

Not carried over: the `h5file` validity filter (h5py is not in this image: a config that
sets it raises) and tqdm/loguru progress output.
"""
from __future__ import annotations

import random
from collections import deque
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np
import torch

from . import _lib
from ._decode import decode as _decode, decode_into as _decode_into, decode_many as _decode_many


class ImageLoader:
    """facenet.py:45-54: read_file + decode_image(channels=3) + resize_with_crop_or_pad(size, size).  `decode` is the host
    half (PIL), the crop/pad runs on the GPU; `loader(path)` returns the uint8 [size, size, 3] device tensor."""

    def __init__(self, config=None):
        self.height = config.size
        self.width = config.size
        if self.height != self.width or not self.height:
            raise ValueError("ImageLoader: config.size must be a positive integer")

    decode = staticmethod(_decode)

    def __call__(self, path):
        return crop_or_pad_batch([self.decode(path)], self.height)[0]


def _pack_ragged(arrays, staging, extra: int = 0):
    """Pack a ragged list of HWC uint8 arrays into (pinned) host staging: int64 byte offsets, int32 (h, w) pairs, `extra`
    bytes for the caller, then the pixels back to back.  Returns (staging, meta = bytes in front of the pixels, total pixel
    bytes)."""
    n = len(arrays)
    hw = np.empty((n, 2), np.int32)
    off = np.empty(n, np.int64)
    total = 0
    for i, a in enumerate(arrays):
        if a.ndim != 3 or a.shape[2] != 3 or a.dtype != np.uint8:
            raise ValueError(f"image {i}: expected HWC uint8 with 3 channels, got {a.dtype} {a.shape}")
        hw[i] = a.shape[:2]
        off[i] = total
        total += a.size
    meta = 8 * n + 8 * n + extra                           # offsets (i64) then hw (2 x i32) in front of the pixels
    if staging is None or staging.numel() < meta + total:
        staging = torch.empty(meta + total, dtype=torch.uint8).pin_memory() if torch.cuda.is_available() else \
            torch.empty(meta + total, dtype=torch.uint8)
    host = staging.numpy()
    host[:8 * n] = off.view(np.uint8)
    host[8 * n:16 * n] = hw.reshape(-1).view(np.uint8)
    for i, a in enumerate(arrays):
        host[meta + off[i]:meta + off[i] + a.size] = a.reshape(-1)
    return staging, meta, total


def crop_or_pad_batch(arrays, size: int, device="cuda", stream=None, staging=None) -> torch.Tensor:
    """Ragged list of HWC uint8 arrays -> uint8 [N, size, size, 3] on the device (one H2D copy + one launch)."""
    lib = _lib.load()
    n = len(arrays)
    if n == 0:
        return torch.empty(0, size, size, 3, dtype=torch.uint8, device=device)
    staging, meta, total = _pack_ragged(arrays, staging)
    st = stream if stream is not None else torch.cuda.current_stream()
    with torch.cuda.stream(st):
        dev = staging[:meta + total].to(device, non_blocking=True)
        out = torch.empty(n, size, size, 3, dtype=torch.uint8, device=device)
        _lib.check(lib.fn_crop_or_pad_u8(dev.data_ptr() + meta, dev.data_ptr(), dev.data_ptr() + 8 * n, out.data_ptr(), n, size,
                                         st.cuda_stream))
    out._staging = staging          # kept alive (and reusable) until the batch is dropped
    return out


# ---- training-time augmentation (image.random_crop / random_flip / random_rotate) ----------------------
AUGMENT_PARAM = np.dtype([("y0", "<i4"), ("x0", "<i4"), ("flip", "<i4"), ("cos", "<f4"), ("sin", "<f4")])   # fn_augment_param
AUGMENT_DRAW = np.dtype([("theta", "<f8"), ("ry", "<i8"), ("rx", "<i8"), ("flip", "?")])
AUGMENT_KEYS = ("random_crop", "random_flip", "random_rotate")


class Augmentation:
    """The three augmentation switches of the reference's training config (apps/configs/train_softmax.yaml:85-91), which the
    reference documents but never reads.  Owns a np.random.Generator seeded by `seed`; `draw(n)` takes the next n per-image
    tuples (theta, r_y, r_x, flip) from it.  Every image consumes four doubles of Generator.random, whatever keys are on:
    theta = 20 u0 - 10 degrees, r_y = floor(2^31 u1), r_x = floor(2^31 u2), flip = u3 < 1/2; a key that is off cancels its
    own effect (theta 0, centre offsets (r = -1), no flip).  Turning one key on therefore leaves the others' draws alone."""

    MAX_DEGREES = 10.0

    def __init__(self, random_crop: bool = False, random_flip: bool = False, random_rotate: bool = False, seed: int = 0):
        self.random_crop, self.random_flip, self.random_rotate = bool(random_crop), bool(random_flip), bool(random_rotate)
        self.seed = seed
        self.rng = np.random.default_rng(seed)

    @classmethod
    def from_config(cls, image_cfg, seed: int):
        """`cfg.image` -> Augmentation, or None when every key is off or missing (the pipeline then runs the plain crop)."""
        keys = {k: bool(getattr(image_cfg, k)) for k in AUGMENT_KEYS}
        return cls(**keys, seed=seed) if any(keys.values()) else None

    def __repr__(self):
        on = [k for k in AUGMENT_KEYS if getattr(self, k)]
        return f"Augmentation({', '.join(on) or 'none'}; seed {self.seed})"

    def draw(self, n: int) -> np.ndarray:
        u = self.rng.random((n, 4))
        d = np.empty(n, AUGMENT_DRAW)
        d["theta"] = (20.0 * u[:, 0] - self.MAX_DEGREES) if self.random_rotate else 0.0
        d["ry"] = np.floor(u[:, 1] * 2.0 ** 31) if self.random_crop else -1
        d["rx"] = np.floor(u[:, 2] * 2.0 ** 31) if self.random_crop else -1
        d["flip"] = (u[:, 3] < 0.5) & self.random_flip
        return d


def augment_params(draws: np.ndarray, hw, size: int) -> np.ndarray:
    """Resolve draws against the decoded sources' (h, w): one fn_augment_param record per image.  Per axis, a source no larger
    than `size` is centred with zero padding (offset -((size - h) // 2)); a larger one is cropped at r % (h - size + 1), or at
    the centre (h - size) // 2 when the draw is -1 (random_crop off).  cos / sin are computed in float64 and stored as float32."""
    hw = np.asarray(hw, np.int64).reshape(-1, 2)
    if len(hw) != len(draws):
        raise ValueError(f"{len(draws)} draws for {len(hw)} images")
    p = np.zeros(len(draws), AUGMENT_PARAM)
    for axis, (field, r) in enumerate((("y0", draws["ry"]), ("x0", draws["rx"]))):
        over = hw[:, axis] - size
        crop = np.where(r >= 0, r % np.maximum(over + 1, 1), over // 2)
        p[field] = np.where(over > 0, crop, -((size - hw[:, axis]) // 2))
    p["flip"] = draws["flip"]
    rad = np.deg2rad(draws["theta"])
    p["cos"], p["sin"] = np.cos(rad), np.sin(rad)
    return p


def augment_batch(arrays, size: int, params: np.ndarray, device="cuda", stream=None, staging=None) -> torch.Tensor:
    """crop_or_pad_batch with per-image augmentation records (AUGMENT_PARAM, e.g. from augment_params): ragged HWC uint8 arrays
    -> uint8 [N, size, size, 3] on the device through fn_augment_u8 (one H2D copy + one launch)."""
    lib = _lib.load()
    n = len(arrays)
    params = np.ascontiguousarray(params)
    if params.dtype != AUGMENT_PARAM or params.shape != (n,):
        raise ValueError(f"expected {n} records of dtype AUGMENT_PARAM, got {params.dtype} {params.shape}")
    if n == 0:
        return torch.empty(0, size, size, 3, dtype=torch.uint8, device=device)
    staging, meta, total = _pack_ragged(arrays, staging, extra=params.nbytes)
    staging.numpy()[16 * n:meta] = params.view(np.uint8)
    st = stream if stream is not None else torch.cuda.current_stream()
    with torch.cuda.stream(st):
        dev = staging[:meta + total].to(device, non_blocking=True)
        out = torch.empty(n, size, size, 3, dtype=torch.uint8, device=device)
        _lib.check(lib.fn_augment_u8(dev.data_ptr() + meta, dev.data_ptr(), dev.data_ptr() + 8 * n, dev.data_ptr() + 16 * n,
                                     out.data_ptr(), n, size, st.cuda_stream))
    out._staging = staging
    return out


class ImageClass:
    """Stores the paths to images for a given class (dataset.py:104-142)."""

    def __init__(self, config):
        if not config.path:
            raise ValueError("Path to download dataset does not specified.")
        self.path = Path(config.path).expanduser()
        self.name = self.path.stem
        if not self.path.exists():
            raise ValueError(f"Directory {self.path} does not exist")
        files = [f for f in self.path.glob("*") if f.is_file()]
        if config.h5file:
            raise NotImplementedError("h5file validity filter: h5py is not available in this build")
        if config.max_nrof_images and len(files) > config.max_nrof_images:
            files = list(np.random.choice(files, size=config.max_nrof_images, replace=False))
        self.files = sorted(str(f) for f in files)

    def __repr__(self):
        return f"{self.__class__.__name__} ({self.name}/{self.nrof_images})"

    @property
    def nrof_images(self):
        return len(self.files)

    @property
    def nrof_pairs(self):
        return self.nrof_images * (self.nrof_images - 1) // 2


class Database:
    """Directory-per-class data set (dataset.py:145-231)."""

    def __init__(self, config):
        if not config.path:
            raise ValueError("Path to download dataset does not specified.")
        self.path = Path(config.path).expanduser()
        if not self.path.exists():
            raise ValueError(f"Directory {self.path} does not exist")
        self.h5file = Path(config.h5file).expanduser() if config.h5file else config.h5file
        dirs = [p for p in self.path.glob("*") if p.is_dir()]
        if config.nrof_classes and len(dirs) > config.nrof_classes:
            dirs = list(np.random.choice(dirs, size=config.nrof_classes, replace=False))
        dirs.sort()
        self.classes = []
        for path in dirs:
            config.path = path                      # the reference mutates the config the same way (dataset.py:170)
            images = ImageClass(config)
            if images.nrof_images > 0:
                self.classes.append(images)

    def __repr__(self):
        return (f"{self.__class__.__name__}\n" + f"{self.path}\n" + f"h5 file {self.h5file}\n" +
                f"Number of classes {self.nrof_classes} \n" + f"Number of images {self.nrof_images}\n" +
                f"Minimal number of images in class {self.min_nrof_images}\n" +
                f"Maximal number of images in class {self.max_nrof_images}\n")

    @property
    def files(self):
        return [f for cls in self.classes for f in cls.files]

    @property
    def labels(self):
        return np.array([idx for idx, cls in enumerate(self.classes) for _ in range(cls.nrof_images)])

    @property
    def min_nrof_images(self):
        return min(cls.nrof_images for cls in self.classes)

    @property
    def max_nrof_images(self):
        return max(cls.nrof_images for cls in self.classes)

    @property
    def nrof_classes(self):
        return len(self.classes)

    @property
    def nrof_images(self):
        return sum(cls.nrof_images for cls in self.classes)

    @property
    def nrof_images_per_class(self):
        return [cls.nrof_images for cls in self.classes]

    def tf_dataset_api(self, loader, batch_size, buffer_size=None, repeat=False, augment=None, resident=None, **kw):
        return tf_dataset_api(self.files, self.labels, loader, batch_size, buffer_size=buffer_size, repeat=repeat, augment=augment,
                              resident=resident, **kw)


class BatchPipeline:
    """Iterable of (uint8 [B,size,size,3] device tensor, int64 [B] device tensor).

    `plan()` yields (files, labels) per batch; decode runs in `workers` threads -- or, with `processes=True`, in that
    many spawned worker processes (PIL decode holds the GIL for part of its work; processes scale with the cores) --
    `prefetch` batches are in flight, the H2D copy and the crop/pad launch go to a side stream and the consumer's current
    stream waits on the batch's event.  Worker processes never touch the GPU (they import facenet_amd._decode only).

    With an `augment` (Augmentation), every batch takes its per-image draws when its plan is pulled (in the parent, in plan
    order, so the batches depend on the seed and the file order only), resolves them once the decoded shapes are known and
    launches fn_augment_u8 instead of fn_crop_or_pad_u8.  With augment=None nothing changes."""

    CHUNK = 10      # files per worker task in process mode

    def __init__(self, plan, loader: ImageLoader, cardinality=None, workers=8, prefetch=2, device="cuda", processes=False,
                 max_image_bytes: int = 300 * 300 * 3, augment: Augmentation = None):
        self._plan, self.loader, self._card, self.augment = plan, loader, cardinality, augment
        self.workers, self.prefetch, self.device, self.processes = workers, max(1, prefetch), device, processes
        self.max_image_bytes = (int(max_image_bytes) + 15) // 16 * 16
        self._pool = None
        self._slots = []          # process mode: shared-memory staging blocks (pinned), one per batch in flight

    # ---- process mode: workers decode straight into pinned shared memory --------------------------------------------------
    def _new_slot(self, nbytes: int):
        from multiprocessing import shared_memory
        shm = shared_memory.SharedMemory(create=True, size=nbytes)
        t = torch.frombuffer(shm.buf, dtype=torch.uint8)
        rc = torch.cuda.cudart().cudaHostRegister(t.data_ptr(), nbytes, 0)      # pinned: the H2D copy can be asynchronous
        return {"shm": shm, "tensor": t, "pinned": int(rc) == 0, "bytes": nbytes}

    def _free_slots(self):
        for s in self._slots:
            try:
                if s["pinned"]:
                    torch.cuda.cudart().cudaHostUnregister(s["tensor"].data_ptr())
                s["tensor"] = None
                s["shm"].close()
                s["shm"].unlink()
            except Exception:
                pass
        self._slots = []

    def _executor(self):
        if self._pool is None:
            if self.processes:
                import multiprocessing
                from concurrent.futures import ProcessPoolExecutor
                self._pool = ProcessPoolExecutor(self.workers, mp_context=multiprocessing.get_context("spawn"))
            else:
                self._pool = ThreadPoolExecutor(self.workers)
        return self._pool

    def close(self):
        if self._pool is not None:
            self._pool.shutdown(wait=self.processes, cancel_futures=True)
            self._pool = None
        self._free_slots()

    def __del__(self):
        self.close()

    def cardinality(self):
        return self._card          # None = infinite (tf.data.INFINITE_CARDINALITY)

    def __len__(self):
        if self._card is None:
            raise TypeError("infinite pipeline")
        return self._card

    def _iter_shared(self):
        """Process mode with the stock decoder: each batch owns a shared-memory slot with a fixed stride per image; the workers
        write pixels into it and return only (h, w), the parent issues ONE H2D copy of the slot and the crop/pad launch.
        Nothing is pickled or repacked on the way (the parent thread was the bottleneck at ~11 000 images/s before)."""
        lib = _lib.load()
        pool = self._executor()
        side = torch.cuda.Stream(device=self.device)
        size = self.loader.height
        pending, free = deque(), list(range(len(self._slots)))
        plan = iter(self._plan())

        def submit():
            # a local stride: the batch being consumed keeps the stride it was decoded with, even when an earlier batch grew it
            try:
                files, labels = next(plan)
            except StopIteration:
                return False
            stride = self.max_image_bytes
            need = stride * len(files)
            k = next((i for i in free if self._slots[i]["bytes"] >= need), None)
            if k is None:
                self._slots.append(self._new_slot(max(need, stride * 128)))
                k = len(self._slots) - 1
            else:
                free.remove(k)
            name = self._slots[k]["shm"].name
            futs = [pool.submit(_decode_into, name, stride, i, files[i:i + self.CHUNK]) for i in range(0, len(files), self.CHUNK)]
            draws = self.augment.draw(len(files)) if self.augment is not None else None
            pending.append((futs, labels, k, len(files), stride, draws))
            return True

        try:
            for _ in range(self.prefetch):
                if not submit():
                    break
            while pending:
                futs, labels, k, n, stride, draws = pending.popleft()
                res = [r for f in futs for r in f.result()]
                submit()
                slot = self._slots[k]
                if any(arr is not None for _, _, arr in res):
                    # an image larger than the stride came back as an array: this batch takes the packing path, and the
                    # stride grows so that later batches fit (slots are re-created on demand)
                    arrays = [arr if arr is not None else
                              np.frombuffer(slot["shm"].buf, np.uint8, count=h * w * 3, offset=i * stride).reshape(h, w, 3).copy()
                              for i, (h, w, arr) in enumerate(res)]
                    if draws is None:
                        images = crop_or_pad_batch(arrays, size, self.device, side)
                    else:
                        images = augment_batch(arrays, size, augment_params(draws, [a.shape[:2] for a in arrays], size), self.device, side)
                    del images._staging
                    with torch.cuda.stream(side):
                        lab = torch.as_tensor(np.asarray(labels, np.int64)).to(self.device)
                    self.max_image_bytes = stride = (max(a.size for a in arrays) + 15) // 16 * 16
                else:
                    hw = torch.tensor([[h, w] for h, w, _ in res], dtype=torch.int32)
                    off = torch.arange(n, dtype=torch.int64) * stride
                    with torch.cuda.stream(side):
                        dev = slot["tensor"][:n * stride].to(self.device, non_blocking=slot["pinned"])
                        d_hw, d_off = hw.to(self.device), off.to(self.device)
                        images = torch.empty(n, size, size, 3, dtype=torch.uint8, device=self.device)
                        if draws is None:
                            _lib.check(lib.fn_crop_or_pad_u8(dev.data_ptr(), d_off.data_ptr(), d_hw.data_ptr(), images.data_ptr(), n, size,
                                                             side.cuda_stream))
                        else:
                            params = augment_params(draws, hw.numpy(), size)
                            d_prm = torch.from_numpy(params.view(np.uint8)).to(self.device)
                            _lib.check(lib.fn_augment_u8(dev.data_ptr(), d_off.data_ptr(), d_hw.data_ptr(), d_prm.data_ptr(), images.data_ptr(),
                                                         n, size, side.cuda_stream))
                        lab = torch.as_tensor(np.asarray(labels, np.int64)).to(self.device)
                done = torch.cuda.Event()
                done.record(side)
                torch.cuda.current_stream().wait_event(done)
                for t in (images, lab):
                    t.record_stream(torch.cuda.current_stream())
                done.synchronize()                              # the slot is reusable once its copy has run
                free.append(k)
                yield images, lab
        finally:
            for futs, *_ in pending:
                for f in futs:
                    f.cancel()

    def __iter__(self):
        if self.processes and type(self.loader).decode is _decode:
            yield from self._iter_shared()
            return
        pool = self._executor()
        decode_many = type(self.loader).decode is _decode and self.processes
        side = torch.cuda.Stream(device=self.device)
        pending, free = deque(), []
        plan = iter(self._plan())

        def submit():
            try:
                files, labels = next(plan)
            except StopIteration:
                return False
            if decode_many:
                futs = [pool.submit(_decode_many, files[i:i + self.CHUNK]) for i in range(0, len(files), self.CHUNK)]
            else:
                futs = [pool.submit(self.loader.decode, f) for f in files]
            draws = self.augment.draw(len(files)) if self.augment is not None else None
            pending.append((futs, labels, draws))
            return True

        try:
            for _ in range(self.prefetch):
                if not submit():
                    break
            while pending:
                futs, labels, draws = pending.popleft()
                arrays = [a for f in futs for a in f.result()] if decode_many else [f.result() for f in futs]
                submit()
                need = sum(a.size for a in arrays) + (16 if draws is None else 16 + AUGMENT_PARAM.itemsize) * len(arrays)
                k = next((i for i, s in enumerate(free) if s.numel() >= need), None)
                staging = free.pop(k) if k is not None else None
                if draws is None:
                    images = crop_or_pad_batch(arrays, self.loader.height, self.device, side, staging)
                else:
                    params = augment_params(draws, [a.shape[:2] for a in arrays], self.loader.height)
                    images = augment_batch(arrays, self.loader.height, params, self.device, side, staging)
                with torch.cuda.stream(side):
                    lab = torch.as_tensor(np.asarray(labels, np.int64)).to(self.device, non_blocking=True)
                done = torch.cuda.Event()
                done.record(side)
                torch.cuda.current_stream().wait_event(done)
                images.record_stream(torch.cuda.current_stream())
                lab.record_stream(torch.cuda.current_stream())
                done.synchronize()                  # the pinned staging buffer is free again once the copy has run
                free.append(images._staging)
                del images._staging
                yield images, lab
        finally:
            for futs, *_ in pending:
                for f in futs:
                    f.cancel()


class ResidentPipeline:
    """BatchPipeline's protocol over a facenet_amd.resident.ResidentDataset: the same `plan()` callables,
    the same (uint8 [B,size,size,3], int64 [B]) device tensors, `cardinality()`, `__len__`, `close()` -- and no decode.  Per
    batch the plan is pulled and the augmentation draws are taken at that moment, in plan order and `prefetch` plans ahead as
    BatchPipeline does, so for the same seeds of `random`, `np.random` and the Augmentation the batches are BatchPipeline's bit
    for bit.  Files become rows, the draws are resolved against the store's host (h, w), and labels, records and rows go into
    one slot of a small pinned ring: one asynchronous H2D copy and one fn_resident_batch_u8 launch on the consumer's current
    stream.  The host waits only for a slot's event when the ring wraps."""

    RING = 4

    def __init__(self, plan, loader: ImageLoader, cardinality=None, resident=None, augment: Augmentation = None, prefetch=2):
        if resident is None:
            raise ValueError("ResidentPipeline needs a ResidentDataset")
        self._plan, self.loader, self._card, self.resident, self.augment = plan, loader, cardinality, resident, augment
        self.prefetch, self.device = max(1, prefetch), resident.device

    def close(self):
        pass

    def cardinality(self):
        return self._card

    def __len__(self):
        if self._card is None:
            raise TypeError("infinite pipeline")
        return self._card

    def __iter__(self):
        store, size = self.resident, self.loader.height
        rec = 8 + AUGMENT_PARAM.itemsize + 4          # per image: int64 label, augmentation record, int32 row
        ring = [{"host": None, "event": None} for _ in range(self.RING)]
        pending, turn = deque(), 0
        plan = iter(self._plan())

        def submit():
            try:
                files, labels = next(plan)
            except StopIteration:
                return False
            pending.append((files, labels, self.augment.draw(len(files)) if self.augment is not None else None))
            return True

        for _ in range(self.prefetch):
            if not submit():
                break
        while pending:
            files, labels, draws = pending.popleft()
            submit()
            n = len(files)
            rows = store.rows_of(files)                # KeyError before anything is launched
            slot, turn = ring[turn % self.RING], turn + 1
            if slot["event"] is not None:
                slot["event"].synchronize()            # the ring wrapped: this slot's copy must have left the host
            if slot["host"] is None or slot["host"].numel() < rec * n:
                slot["host"] = torch.empty(rec * max(n, 256), dtype=torch.uint8).pin_memory()
            host = slot["host"].numpy()
            host[:8 * n] = np.asarray(labels, np.int64).view(np.uint8)
            if draws is not None:
                host[8 * n:28 * n] = augment_params(draws, store.host_hw[rows], size).view(np.uint8)
            host[28 * n:32 * n] = rows.view(np.uint8)
            st = torch.cuda.current_stream(self.device)
            dev = slot["host"][:rec * n].to(self.device, non_blocking=True)
            slot["event"] = torch.cuda.Event()
            slot["event"].record(st)
            images = torch.empty(n, size, size, 3, dtype=torch.uint8, device=self.device)
            store.launch(dev.data_ptr() + 28 * n, dev.data_ptr() + 8 * n if draws is not None else 0, images, n, size, st)
            yield images, dev[:8 * n].view(torch.int64)


def tf_dataset_api(files, labels, loader, batch_size, buffer_size=None, repeat=False, augment=None, resident=None, **kw):
    """dataset.py:15-43: zip(files, labels) -> optional shuffle -> optional repeat -> batch -> prefetch.  With a
    `buffer_size` the reference shuffles once globally and then through a buffer_size*batch_size window, reshuffled
    every iteration; here every epoch is a fresh full permutation (the window's limit case).  `repeat` comes before
    `batch` as in the reference, so a repeating stream has full batches that span epochs and only a finite one ends short.
    `augment`: an Augmentation for training batches (BatchPipeline), None for the plain centre crop / pad.
    `resident`: a ResidentDataset holding `files` -> a ResidentPipeline over the same plan (`workers` / `processes` are ignored)."""
    files, labels = list(files), list(np.asarray(labels).tolist())
    if len(files) != len(labels):
        raise ValueError("files and labels differ in length")
    n = len(files)

    def plan():
        bf, bl = [], []
        while True:
            order = np.random.permutation(n) if buffer_size is not None else np.arange(n)
            for i in order:
                bf.append(files[i])
                bl.append(labels[i])
                if len(bf) == batch_size:
                    yield bf, bl
                    bf, bl = [], []
            if not repeat:                       # repeat() sits before batch(): only a finite stream has a short batch
                if bf:
                    yield bf, bl
                return

    card = None if repeat else (n + batch_size - 1) // batch_size
    if resident is not None:
        return ResidentPipeline(plan, loader, card, resident, augment=augment, prefetch=kw.get("prefetch", 2))
    return BatchPipeline(plan, loader, card, augment=augment, **kw)


def pipeline_with_equal_batches(loader, classes, config, augment=None, resident=None, **kw):
    """dataset.py:46-101: endless P x K batches, 20 random classes x 5 random files each (the reference overwrites the
    two config values the same way, :61-62); labels are class indexes.  Raises ValueError (from random.sample) when there
    are fewer classes / files than asked for, as the reference's generator does.  `augment` and `resident` as for tf_dataset_api."""
    config.nrof_classes_per_batch = 20
    config.nrof_examples_per_class = 5
    for idx, _class in enumerate(classes):
        _class.index = idx

    def plan():
        while True:
            _files, _indexes = [], []
            for cls in random.sample(classes, config.nrof_classes_per_batch):
                _files += random.sample(cls.files, config.nrof_examples_per_class)
                _indexes += [cls.index] * config.nrof_examples_per_class
            yield _files, _indexes

    if resident is not None:
        return ResidentPipeline(plan, loader, None, resident, augment=augment, prefetch=kw.get("prefetch", 2))
    return BatchPipeline(plan, loader, None, augment=augment, **kw)
