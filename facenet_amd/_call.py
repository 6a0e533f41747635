"""What every host wrapper of a fn_* entry needs around the ctypes call itself: pointers, the stream,
the fp32 table of a set of embeddings, a workspace of the size the library asks for, the `range` words of the pair kernels and the
check of an integer argument.  Each is defined here and nowhere else; only `_lib` is imported, so using one pulls in no network."""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib


def ptr(t, elem_off: int = 0):
    """The address of element ``elem_off`` of a tensor; None stays None (the C ABI's optional arguments)."""
    return None if t is None else t.data_ptr() + elem_off * t.element_size()


def stream(device=None) -> int:
    """The handle of the current stream of ``device`` (None: of the current device)."""
    return torch.cuda.current_stream(device).cuda_stream


def host_array(x) -> np.ndarray:
    """A tensor (wherever it lives) or anything array-like -> NumPy on the host."""
    return np.asarray(x.cpu() if torch.is_tensor(x) else x)


def as_table(x, device) -> torch.Tensor:
    """fp32 [n, E] contiguous on `device`, rows 16-byte aligned (E % 4 == 0 is required by the kernels)."""
    t = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    if t.dim() != 2:
        raise ValueError(f"embeddings must be a 2-D [n, E] array, got shape {tuple(t.shape)}")
    if t.shape[1] % 4:
        raise ValueError(f"embedding length {t.shape[1]} must be a multiple of 4")
    t = t.to(device=device, dtype=torch.float32).contiguous()
    if t.data_ptr() % 16:
        t = t.clone()
    return t


def workspace_size(sizer, what, *args) -> int:
    """What sizer(*args, &size), a fn_*_workspace entry, reports (bytes, or the words of the entry's own unit)."""
    size = ctypes.c_longlong(0)
    _lib.check(sizer(*args, ctypes.byref(size)), what)
    return size.value


def workspace(device, sizer, what, *args) -> torch.Tensor:
    """The int64 workspace tensor of the bytes that `workspace_size` reports (at least 8)."""
    return torch.empty(max(1, (workspace_size(sizer, what, *args) + 7) // 8), dtype=torch.int64, device=device)


def _decode_ord(i: int) -> float:
    i = int(i)
    bits = i if i >= 0 else (i ^ 0x7FFFFFFF)
    return float(np.array([bits & 0xFFFFFFFF], dtype=np.uint32).view(np.float32)[0])


def check_unit_range(rng_words, atol):
    """The two `range` words of a kernel (a device tensor; reading them waits for the kernel) -> the reference's ValueError when
    some dot product left +-(1 + atol) (statistics.py:40-42).  A kernel that evaluated no pair leaves words that decode to
    lo = +3.4e38 > hi = -3.4e38, which neither comparison takes for a violation: the empty case needs no rule of its own."""
    lo, hi = (_decode_ord(v) for v in rng_words.cpu().tolist())
    if lo < -(1 + atol) or hi > 1 + atol:
        raise ValueError("\nembeddings must be normalized to 1, range {} {}".format(lo, hi))


def check_int(name, value, lo, hi=None, note="") -> int:
    """``value`` as an int when it is an integer (no bool, no float) in [lo, hi] (hi None: no upper end), else the ValueError
    that names the rule; ``note`` follows the rule in the message."""
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or value < lo or (hi is not None and value > hi):
        rule = f"an integer in [{lo}, {hi}]" if hi is not None else "a non-negative integer" if lo == 0 else f"an integer of at least {lo}"
        raise ValueError(f"{name} must be {rule}{note}, got {value!r}")
    return int(value)
