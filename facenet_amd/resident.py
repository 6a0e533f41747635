"""The decoded training set in device memory.

Two halves.  The *pack* is a directory on disk with the decoded HWC uint8 pixels of a `Database` (`pixels.u8`, images back
to back in `Database.files` order, each starting at a multiple of 16 bytes) and their tables (`index.npz`), so that a data
set is decoded once and not once per epoch and rank; it is host-only code (NumPy, PIL).  `ResidentDataset` is the same
layout in one device tensor, uploaded through two pinned staging buffers, and `batch()` builds a [N, size, size, 3] batch
from it by row number in one launch (`fn_resident_batch_u8`), with the augmentation records of `fn_augment_u8` or the plain
centre crop / pad.  Both are written and read in bounded chunks: the whole set never sits in host memory.
"""
from __future__ import annotations

import os
import time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np
import torch

from . import _lib
from ._decode import decode as _decode

VERSION = 1
ALIGN = 16                         # every image of a pack starts at a multiple of this many bytes
PIXELS, INDEX = "pixels.u8", "index.npz"
CHUNK_BYTES = 64 << 20             # one staging buffer / one window of decoded images in flight


class PackVersionError(ValueError):
    """index.npz was written by another format version."""


def _aligned(n: int, align: int) -> int:
    return (n + align - 1) // align * align


def _stat(files):
    st = [os.stat(f) for f in files]
    return np.array([s.st_size for s in st], np.int64), np.array([s.st_mtime_ns for s in st], np.int64)


def _relative(dbase):
    """(absolute file list, the same paths relative to the data set's root) in Database.files order."""
    files = dbase.files
    return files, [os.path.relpath(f, dbase.path) for f in files]


def _decoded(files, workers: int, chunk_bytes: int = CHUNK_BYTES):
    """Yield the decoded array of every file, in order, decoding `workers` at a time in windows whose decoded bytes stay
    near `chunk_bytes` (the window is sized from the largest image seen so far)."""
    i, window, largest = 0, max(1, 4 * workers), 1
    with ThreadPoolExecutor(max(1, workers)) as pool:
        while i < len(files):
            arrays = list(pool.map(lambda f: _decode(f), files[i:i + window]))      # the module's _decode, looked up per call
            i += len(arrays)
            for a in arrays:
                if a.ndim != 3 or a.shape[2] != 3 or a.dtype != np.uint8:
                    raise ValueError(f"expected HWC uint8 with 3 channels, got {a.dtype} {a.shape}")
                largest = max(largest, a.size)
                yield a
            window = int(min(4096, max(workers, chunk_bytes // largest)))


# ---- the pack on disk ------------------------------------------------------------------------------------------------------------
class Pack:
    """An opened pack: `pixels` is an np.memmap, the rest are the arrays of index.npz."""

    def __init__(self, path):
        self.path = Path(path)
        with np.load(self.path / INDEX, allow_pickle=False) as z:
            self.version = int(z["version"])
            if self.version != VERSION:
                raise PackVersionError(f"{self.path}: pack format version {self.version}, this build reads version {VERSION}")
            self.files = [str(f) for f in z["files"]]
            self.labels = z["labels"].astype(np.int64)
            self.classes = [str(c) for c in z["classes"]]
            self.hw = z["hw"].astype(np.int32).reshape(-1, 2)
            self.offsets = z["offsets"].astype(np.int64)
            self.st_size, self.st_mtime_ns = z["st_size"].astype(np.int64), z["st_mtime_ns"].astype(np.int64)
        m = len(self.files)
        if not (len(self.labels) == len(self.hw) == len(self.st_size) == len(self.st_mtime_ns) == m and len(self.offsets) == m + 1):
            raise ValueError(f"{self.path}: index tables disagree in length")
        have = os.path.getsize(self.path / PIXELS)
        if have < int(self.offsets[m]):
            raise ValueError(f"{self.path}: {PIXELS} holds {have} bytes, the index needs {int(self.offsets[m])}")
        self.pixels = np.memmap(self.path / PIXELS, dtype=np.uint8, mode="r", shape=(int(self.offsets[m]),)) if m and self.offsets[m] \
            else np.zeros(0, np.uint8)

    @property
    def nrof_images(self):
        return len(self.files)

    @property
    def nbytes(self):
        return int(self.offsets[-1])

    def image(self, i: int) -> np.ndarray:
        h, w = self.hw[i]
        o = int(self.offsets[i])
        return np.asarray(self.pixels[o:o + int(h) * int(w) * 3]).reshape(h, w, 3)

    def matches(self, dbase) -> bool:
        """Valid for `dbase` exactly when the relative file list, the labels and every file's recorded size and mtime match
        (the version was checked on opening)."""
        files, rel = _relative(dbase)
        if rel != self.files or not np.array_equal(np.asarray(dbase.labels, np.int64), self.labels):
            return False
        size, mtime = _stat(files)
        return np.array_equal(size, self.st_size) and np.array_equal(mtime, self.st_mtime_ns)


def build_pack(dbase, path, workers: int = 8, log=None) -> Pack:
    """Decode `dbase` into the pack directory `path`.  Everything is written under a temporary name beside it and renamed at
    the end, so an interrupted build is never taken for a whole pack; an earlier pack at `path` is replaced."""
    path = Path(path).expanduser()
    files, rel = _relative(dbase)
    m = len(files)
    size, mtime = _stat(files)                    # taken before the decode: a file changed meanwhile invalidates the pack
    tmp = path.parent / f"{path.name}.tmp.{os.getpid()}"
    path.parent.mkdir(parents=True, exist_ok=True)
    _remove_pack(tmp)
    tmp.mkdir()
    hw, offsets = np.zeros((m, 2), np.int32), np.zeros(m + 1, np.int64)
    pos, zeros = 0, bytes(ALIGN)
    with open(tmp / PIXELS, "wb") as f:
        for i, a in enumerate(_decoded(files, workers)):
            hw[i], offsets[i] = a.shape[:2], pos
            f.write(np.ascontiguousarray(a).data)
            end = _aligned(pos + a.size, ALIGN)
            f.write(zeros[:end - pos - a.size])
            pos = end
            if log is not None and (i + 1) % 50000 == 0:
                log(f"packed {i + 1}/{m} images")
    offsets[m] = pos
    with open(tmp / INDEX, "wb") as f:
        np.savez(f, version=np.int64(VERSION), files=np.array(rel, dtype=np.str_), labels=np.asarray(dbase.labels, np.int64),
                 classes=np.array([c.name for c in dbase.classes], dtype=np.str_), hw=hw, offsets=offsets, st_size=size, st_mtime_ns=mtime)
    _remove_pack(path)
    os.rename(tmp, path)
    return Pack(path)


def _remove_pack(path):
    """Remove a pack directory (its two files and the directory); anything else inside it is not ours and makes rmdir raise."""
    path = Path(path)
    if not path.exists():
        return
    for name in (PIXELS, INDEX):
        if (path / name).exists():
            (path / name).unlink()
    path.rmdir()


def ensure_pack(dbase, path, workers: int = 8, log=None):
    """(pack, hit): the pack at `path` when it is valid for `dbase`, else a freshly built one.  A missing pack, another format
    version and any mismatch with the data set rebuild it; a pack whose pixels are shorter than its index raises."""
    path = Path(path).expanduser()
    if (path / INDEX).exists() and (path / PIXELS).exists():
        try:
            pack = Pack(path)
        except PackVersionError:
            pack = None
        if pack is not None and pack.matches(dbase):
            return pack, True
        del pack
    return build_pack(dbase, path, workers=workers, log=log), False


# ---- the store on the device -----------------------------------------------------------------------------------------------------
class _Upload:
    """Sequential writer into a device uint8 tensor through two pinned staging buffers of fixed size: the host fills one while
    the asynchronous copy of the other runs."""

    def __init__(self, pool: torch.Tensor, chunk_bytes: int = CHUNK_BYTES):
        self.pool, self.pos, self.fill, self.k = pool, 0, 0, 0
        chunk_bytes = max(4096, min(int(chunk_bytes), pool.numel()))      # a small store does not pin 2 x 64 MiB
        self.stream = torch.cuda.Stream(device=pool.device)
        self.stream.wait_stream(torch.cuda.current_stream(pool.device))  # the pool's memory may have work queued there
        self.bufs = [torch.empty(chunk_bytes, dtype=torch.uint8).pin_memory() for _ in range(2)]
        self.host = [b.numpy() for b in self.bufs]
        self.events = [None, None]

    def _flush(self):
        if self.fill:
            with torch.cuda.stream(self.stream):
                self.pool[self.pos:self.pos + self.fill].copy_(self.bufs[self.k][:self.fill], non_blocking=True)
                self.events[self.k] = torch.cuda.Event()
                self.events[self.k].record(self.stream)
            self.pos += self.fill
        self.k, self.fill = 1 - self.k, 0
        if self.events[self.k] is not None:
            self.events[self.k].synchronize()           # the buffer about to be filled has left the host

    def write(self, data: np.ndarray):
        """Append the bytes of a flat uint8 array (any length, split over staging buffers as needed)."""
        done = 0
        while done < data.size:
            room = self.host[self.k].size - self.fill
            if room == 0:
                self._flush()
                continue
            n = min(room, data.size - done)
            self.host[self.k][self.fill:self.fill + n] = data[done:done + n]
            self.fill += n
            done += n

    def skip_to(self, pos: int):
        """Zero bytes up to absolute position `pos` (alignment gaps)."""
        gap = pos - (self.pos + self.fill)
        if gap:
            self.write(np.zeros(gap, np.uint8))

    def finish(self):
        self._flush()
        self.stream.synchronize()
        torch.cuda.current_stream(self.pool.device).wait_stream(self.stream)


def _layout(hw: np.ndarray, align: int):
    """int64 offsets [M + 1] of images of (h, w) packed back to back, each start (and the end) a multiple of `align`."""
    sizes = hw[:, 0].astype(np.int64) * hw[:, 1].astype(np.int64) * 3
    offsets = np.zeros(len(hw) + 1, np.int64)
    pos = 0
    for i, s in enumerate(sizes.tolist()):
        offsets[i] = pos
        pos = _aligned(pos + s, align)
    offsets[len(hw)] = pos
    return offsets


def default_max_bytes(device) -> int:
    """Half the device's total memory, as torch.cuda.mem_get_info reports it."""
    return torch.cuda.mem_get_info(torch.device(device))[1] // 2


class ResidentDataset:
    """Decoded pixels of a whole data set in one device tensor, with device tables `offsets` int64 [M], `hw` int32 [M, 2] and
    `labels` int64 [M], and host copies of `hw`, the file list and a file -> row map.  Build it with from_database, from_pack
    or from_arrays."""

    def __init__(self, pool, offsets: np.ndarray, hw: np.ndarray, files, labels, device, info=None):
        self.device = torch.device(device)
        self.pool = pool
        self.host_hw = np.ascontiguousarray(hw, np.int32).reshape(-1, 2)
        self.host_offsets = np.ascontiguousarray(offsets[:len(self.host_hw)], np.int64)
        self.files = [str(f) for f in files]
        self.host_labels = np.asarray(labels, np.int64)
        if not len(self.files) == len(self.host_hw) == len(self.host_labels):
            raise ValueError("files, labels and images differ in number")
        self.offsets = torch.from_numpy(self.host_offsets).to(self.device)
        self.hw = torch.from_numpy(self.host_hw).to(self.device)
        self.labels = torch.from_numpy(self.host_labels).to(self.device)
        self.row = {f: i for i, f in enumerate(self.files)}
        self.info = dict(info or {})                # how it was made: seconds, cache "hit" / "miss" / "none"

    # ---- constructors ------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _allocate(need: int, device, max_bytes):
        device = torch.device(device)
        if device.type != "cuda":
            raise ValueError(f"a resident data set lives on a GPU, not on {device}")
        allowed = default_max_bytes(device) if max_bytes is None else int(max_bytes)
        if need > allowed:
            raise ValueError(f"the resident data set needs {need} bytes of device memory and {allowed} bytes are allowed "
                             "(dataset.resident_bytes; the default is half the device's memory)")
        return torch.empty(max(need, 1), dtype=torch.uint8, device=device)

    @classmethod
    def from_arrays(cls, arrays, files, labels, device="cuda", align: int = ALIGN, max_bytes=None):
        """From decoded HWC uint8 arrays already in host memory; `align` (>= 1) is the alignment of every image's start."""
        for i, a in enumerate(arrays):
            if a.ndim != 3 or a.shape[2] != 3 or a.dtype != np.uint8:
                raise ValueError(f"image {i}: expected HWC uint8 with 3 channels, got {a.dtype} {a.shape}")
        hw = np.array([a.shape[:2] for a in arrays], np.int32).reshape(-1, 2)
        offsets = _layout(hw, max(1, int(align)))
        pool = cls._allocate(int(offsets[-1]), device, max_bytes)
        up = _Upload(pool)
        for a, o in zip(arrays, offsets):
            up.skip_to(int(o))
            up.write(np.ascontiguousarray(a).reshape(-1))
        up.skip_to(int(offsets[-1]))
        up.finish()
        return cls(pool, offsets, hw, files, labels, device, {"cache": "none"})

    @classmethod
    def from_pack(cls, path, device="cuda", max_bytes=None, root=None):
        """From a pack directory.  The pack names its files relative to the data set's root: with `root` the store's file list
        (and rows_of) use root / name, as Database.files does."""
        pack = path if isinstance(path, Pack) else Pack(path)
        t0 = time.perf_counter()
        pool = cls._allocate(pack.nbytes, device, max_bytes)
        up = _Upload(pool)
        step = up.host[0].size
        for a in range(0, pack.nbytes, step):
            up.write(pack.pixels[a:a + step])
        up.finish()
        files = pack.files if root is None else [os.path.join(str(root), f) for f in pack.files]
        return cls(pool, pack.offsets, pack.hw, files, pack.labels, device, {"load_seconds": time.perf_counter() - t0})

    @classmethod
    def from_database(cls, dbase, cache=None, device="cuda", max_bytes=None, workers: int = 8, log=None):
        """With a `cache` directory: load the pack there when it is valid for `dbase`, build it first when not.  Without one:
        decode straight into the device pool (the image sizes are read from the file headers first, so the pool is allocated --
        and refused -- before anything is decoded)."""
        t0 = time.perf_counter()
        if cache:
            pack, hit = ensure_pack(dbase, cache, workers=workers, log=log)
            out = cls.from_pack(pack, device=device, max_bytes=max_bytes, root=dbase.path)
            out.info.update(cache="hit" if hit else "miss", seconds=time.perf_counter() - t0)
            return out
        from PIL import Image
        files = dbase.files

        def header(f):
            with Image.open(f) as im:
                return im.size[1], im.size[0]

        with ThreadPoolExecutor(max(1, workers)) as pool_:
            hw = np.array(list(pool_.map(header, files)), np.int32).reshape(-1, 2)
        offsets = _layout(hw, ALIGN)
        pool = cls._allocate(int(offsets[-1]), device, max_bytes)
        up = _Upload(pool)
        for i, a in enumerate(_decoded(files, workers)):
            if a.shape[:2] != tuple(hw[i]):
                raise ValueError(f"{files[i]}: decoded to {a.shape[:2]}, its header says {tuple(hw[i])}")
            up.skip_to(int(offsets[i]))
            up.write(a.reshape(-1))
        up.skip_to(int(offsets[-1]))
        up.finish()
        return cls(pool, offsets, hw, files, dbase.labels, device, {"cache": "none", "seconds": time.perf_counter() - t0})

    # ---- queries -----------------------------------------------------------------------------------------------------------------
    @property
    def nrof_images(self):
        return len(self.files)

    @property
    def nbytes(self):
        return int(self.pool.numel()) if self.nrof_images else 0

    def __repr__(self):
        return f"{self.__class__.__name__}({self.nrof_images} images, {self.nbytes} bytes on {self.device})"

    def rows_of(self, files) -> np.ndarray:
        """int32 row numbers of `files`; KeyError names the first file the store does not hold."""
        row = self.row
        try:
            return np.fromiter((row[f] for f in files), np.int32, count=len(files))
        except KeyError:
            missing = next(f for f in files if f not in row)
            raise KeyError(f"{missing} is not in the resident data set ({self.nrof_images} images)") from None

    def image(self, i: int) -> np.ndarray:
        """Image `i` read back from the device, as an HWC uint8 host array (for checks)."""
        h, w = (int(v) for v in self.host_hw[i])
        o = int(self.host_offsets[i])
        return self.pool[o:o + h * w * 3].cpu().numpy().reshape(h, w, 3)

    def launch(self, rows_ptr: int, params_ptr: int, out: torch.Tensor, n: int, size: int, stream):
        """fn_resident_batch_u8 on device pointers (params_ptr 0: centre crop / pad).  A refused call raises FacenetHipError."""
        resident_batch_u8(self.pool.data_ptr(), self.offsets.data_ptr(), self.hw.data_ptr(), self.nrof_images, rows_ptr, params_ptr,
                          out.data_ptr(), n, size, stream.cuda_stream)

    def batch(self, rows, size: int, params=None, out=None, stream=None) -> torch.Tensor:
        """uint8 [N, size, size, 3]: image n is row rows[n], augmented by params[n] (records of dataset.AUGMENT_PARAM, as
        fn_augment_u8 takes them) or, with params None, centre-cropped / zero-padded as fn_crop_or_pad_u8 does.  `rows` and
        `params` may be host arrays or device tensors."""
        from . import dataset
        st = stream if stream is not None else torch.cuda.current_stream(self.device)
        with torch.cuda.stream(st):
            if not isinstance(rows, torch.Tensor):
                rows = torch.from_numpy(np.ascontiguousarray(rows, np.int32).reshape(-1))
            rows = rows.to(self.device, torch.int32).contiguous()
            n = rows.numel()
            if params is not None:
                if not isinstance(params, torch.Tensor):
                    params = np.ascontiguousarray(params)
                    if params.dtype != dataset.AUGMENT_PARAM or params.shape != (n,):
                        raise ValueError(f"expected {n} records of dtype AUGMENT_PARAM, got {params.dtype} {params.shape}")
                    params = torch.from_numpy(params.view(np.uint8))
                params = params.to(self.device).contiguous()
                if params.numel() * params.element_size() != n * dataset.AUGMENT_PARAM.itemsize:
                    raise ValueError(f"expected {n} augmentation records, got {params.numel() * params.element_size()} bytes")
            if out is None:
                out = torch.empty(n, size, size, 3, dtype=torch.uint8, device=self.device)
            elif out.shape != (n, size, size, 3) or out.dtype != torch.uint8 or not out.is_contiguous() or out.device != rows.device:
                raise ValueError(f"out must be a contiguous uint8 [{n}, {size}, {size}, 3] tensor on {self.device}")
            if n:
                self.launch(rows.data_ptr(), params.data_ptr() if params is not None else 0, out, n, size, st)
        return out


def resident_batch_u8(pool: int, offsets: int, hw: int, m: int, rows: int, params: int, dst: int, n: int, size: int, stream: int = 0):
    """The C entry on raw device pointers; any refusal (bad arguments, a failed launch) raises FacenetHipError with the library's
    error text."""
    lib = _lib.load()
    rc = lib.fn_resident_batch_u8(pool, offsets, hw, m, rows, params, dst, n, size, stream)
    if rc != 0:
        raise _lib.FacenetHipError(f"fn_resident_batch_u8: rc={rc}: {lib.fn_last_error().decode('utf-8', 'replace')}")


def ensure_pack_collective(dbase, path, rank: int, workers: int = 8):
    """Under an initialised torch.distributed group: rank 0 makes sure of the pack (returning whether it was a hit), the other
    ranks wait at the barrier (returning None) and find it valid afterwards.  Without a group: nothing, None."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
        return None
    hit = ensure_pack(dbase, path, workers=workers)[1] if rank == 0 else None
    dist.barrier()
    return hit


def from_config(dataset_cfg, dbase, device="cuda", rank: int = 0, log=None, workers: int = 8):
    """The store the training apps build for `dataset.resident: true`: dataset.resident_cache names the pack directory (none:
    decode straight to the device), dataset.resident_bytes the cap (none: half the device's memory).  Under torch.distributed
    every rank holds the whole set: rank 0 builds a missing pack, the ranks meet at a barrier and all of them load it.  Rank 0
    logs one line."""
    cache = dataset_cfg.resident_cache if dataset_cfg.resident_cache else None
    cap = int(dataset_cfg.resident_bytes) if dataset_cfg.resident_bytes else None
    t0 = time.perf_counter()
    hit = ensure_pack_collective(dbase, cache, rank, workers=workers) if cache else None
    store = ResidentDataset.from_database(dbase, cache=cache, device=device, max_bytes=cap, workers=workers)
    if hit is not None:
        store.info["cache"] = "hit" if hit else "miss"
    store.info["seconds"] = time.perf_counter() - t0
    if rank == 0 and log is not None:
        how = {"hit": "cache hit", "miss": "cache miss", "none": "no cache"}[store.info["cache"]]
        log(f"resident data set: {store.nrof_images} images, {store.nbytes / 2 ** 30:.3f} GiB in {store.info['seconds']:.1f} s ({how})")
    return store
