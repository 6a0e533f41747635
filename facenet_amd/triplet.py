"""Triplet selection and loss (build-defined: the reference has none; arXiv 1503.03832 sec. 3).
Thin host wrappers over fn_pairwise_sqdist / fn_select_triplets / fn_triplet_loss_fwd_bwd / fn_batch_triplet_fwd_bwd (the
batch-mined losses of arXiv 1703.07737 sec. 2) for use outside a plan."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from ._call import ptr as _ptr, stream


def squared_distances(emb: torch.Tensor) -> torch.Tensor:
    lib = _lib.load()
    e = emb.to(dtype=torch.float32).contiguous()
    n, E = e.shape
    out = torch.empty(n, n, dtype=torch.float32, device=e.device)
    _lib.check(lib.fn_pairwise_sqdist(_ptr(e), _ptr(e), _ptr(out), None, n, n, E, 2, stream(e.device)),
               "pairwise_sqdist")
    return out


def select_triplets(dist: torch.Tensor, labels, alpha: float, nrof_triplets: int, seed: int = 0, semi_hard: bool = False):
    """Returns (triplets int32 [T,3] on device, info dict).  Raises ValueError when the pool has too few positive pairs."""
    lab_host = np.asarray(labels)
    n = dist.shape[0]
    if lab_host.shape != (n,):
        raise ValueError(f"labels must have one entry per row of dist ({n}), got {lab_host.shape}")
    # a pool of one identity has anchor-positive pairs but no negative for any of them: the kernel would leave every triplet slot
    # unwritten and the zero-filled buffer below would pass for a selection
    if len(np.unique(lab_host)) < 2:
        raise ValueError("triplet selection needs at least two identities in the pool: every row carries the same label, so no pair has a negative")
    lib = _lib.load()
    lab = torch.as_tensor(lab_host, dtype=torch.int32).to(dist.device)
    trip = torch.zeros(nrof_triplets, 3, dtype=torch.int32, device=dist.device)
    info = torch.zeros(8 + 5 * (n * (n - 1) // 2), dtype=torch.int32, device=dist.device)
    _lib.check(lib.fn_select_triplets(_ptr(dist.contiguous()), _ptr(lab), n, float(alpha), nrof_triplets, int(seed) & 0xFFFFFFFF,
                                      1 if semi_hard else 0, _ptr(trip), _ptr(info), stream(dist.device)),
               "select_triplets")
    q, valid, short = info[:3].cpu().tolist()
    if short:
        raise ValueError("pool too small for the requested number of triplets")
    return trip, {"pairs": q, "valid": valid}


def triplet_loss(emb: torch.Tensor, alpha: float, with_grad: bool = False):
    """emb fp32 [3T,E] rows (a0,p0,n0,...).  Returns loss (0-d tensor) and, optionally, d loss / d emb."""
    lib = _lib.load()
    e = emb.to(dtype=torch.float32).contiguous()
    T, E = e.shape[0] // 3, e.shape[1]
    loss = torch.zeros(4, dtype=torch.float32, device=e.device)      # word 0 = the loss, words 1-3 = the launch's accumulator
    grad = torch.empty_like(e) if with_grad else None
    _lib.check(lib.fn_triplet_loss_fwd_bwd(_ptr(e), _ptr(grad), _ptr(loss), T, E, float(alpha),
                                           stream(e.device)), "triplet_loss")
    return (loss[0], grad) if with_grad else loss[0]


BATCH_STRATEGIES = {"batch_hard": 0, "batch_all": 1}


def batch_triplet_loss(emb: torch.Tensor, labels, alpha: float = 0.2, strategy: str = "batch_hard", soft: bool = False,
                       with_grad: bool = False):
    """emb fp32 [N,E] (normalised or not), labels [N] identity ids.  Batch-hard or batch-all triplet loss mined inside the batch, with
    the hinge (``alpha``) or the soft margin.  Returns (loss 0-d tensor, info) or (loss, d loss / d emb, info); info = {"anchors",
    "terms", "active", "active_fraction"}.  A non-finite distance makes the loss NaN."""
    if strategy not in BATCH_STRATEGIES:
        raise ValueError(f"unknown strategy {strategy!r}: expected 'batch_hard' or 'batch_all'")
    lib = _lib.load()
    e = emb.to(dtype=torch.float32).contiguous()
    n, E = e.shape
    lab = torch.as_tensor(np.asarray(torch.as_tensor(labels).cpu()).reshape(-1).astype(np.int32)).to(e.device)
    if lab.numel() != n:
        raise ValueError(f"labels must have one entry per row of emb ({n}), got {lab.numel()}")
    if not 2 <= n <= 1024:
        raise ValueError(f"batch_triplet_loss takes 2 to 1024 rows, got {n}")
    dist = squared_distances(e)
    loss = torch.zeros(4, dtype=torch.float32, device=e.device)      # word 0 = the loss, words 1-3 = the launch's
    coef = torch.empty(n, n, dtype=torch.float32, device=e.device)
    info = torch.zeros(8, dtype=torch.int32, device=e.device)
    grad = torch.empty_like(e) if with_grad else None
    _lib.check(lib.fn_batch_triplet_fwd_bwd(_ptr(e), _ptr(dist), _ptr(lab), _ptr(grad), _ptr(loss), _ptr(coef), _ptr(info), n, E,
                                            float(alpha), BATCH_STRATEGIES[strategy], 1 if soft else 0, stream(e.device)), "batch_triplet")
    anchors, terms, active = info[:3].cpu().tolist()
    stats = {"anchors": anchors, "terms": terms, "active": active, "active_fraction": active / terms if terms else 0.0}
    return (loss[0], grad, stats) if with_grad else (loss[0], stats)


XBM_MAX_ROWS = 65536


def memory_stats(info) -> dict:
    """info int32 [8] of fn_xbm_triplet_fwd_bwd as a dict: the counts of batch_triplet_loss plus what the memory contributed."""
    anchors, terms, active, _, mem_pos, mem_neg, valid = (int(v) for v in info[:7])
    return {"anchors": anchors, "terms": terms, "active": active, "active_fraction": active / terms if terms else 0.0,
            "memory_valid": valid, "memory_positives": mem_pos, "memory_negatives": mem_neg}


class CrossBatchMemory:
    """A cross-batch memory (Wang et al., CVPR 2020) for use outside a plan: a ring of the last ``size``
    normalised embeddings and their identity ids on the device, and the batch-hard loss mined over a batch and that ring.  Labels
    must name the same identity in every call.  ``loss`` does not enqueue: call ``enqueue`` after it, so that a step mines against
    earlier steps only."""

    def __init__(self, size: int, E: int, device="cuda"):
        if not 2 <= size <= XBM_MAX_ROWS:
            raise ValueError(f"a cross-batch memory holds 2 to {XBM_MAX_ROWS} rows, got {size}")
        if not 1 <= E <= 512:
            raise ValueError(f"the embedding size must be in [1, 512], got {E}")
        self.size, self.E, self.device = int(size), int(E), torch.device(device)
        self.emb = torch.zeros(self.size, self.E, dtype=torch.float32, device=self.device)
        self.labels = torch.zeros(self.size, dtype=torch.int32, device=self.device)
        self.state = torch.zeros(4, dtype=torch.int32, device=self.device)      # cursor | valid rows | enqueue calls seen | 0

    @property
    def valid(self) -> int:
        return int(self.state[1].item())

    def reset(self):
        """Empty the ring; the call counter restarts too."""
        self.state.zero_()

    def _batch(self, emb, labels):
        e = emb.to(device=self.device, dtype=torch.float32).contiguous()
        n, E = e.shape
        lab = torch.as_tensor(np.asarray(torch.as_tensor(labels).cpu()).reshape(-1).astype(np.int32)).to(self.device)
        if E != self.E or lab.numel() != n:
            raise ValueError(f"expected emb [N,{self.E}] and one label per row, got {tuple(e.shape)} and {lab.numel()} labels")
        if not 1 <= n <= min(self.size, 1024):
            raise ValueError(f"a batch holds 1 to {min(self.size, 1024)} rows (the memory's size or 1024), got {n}")
        embn = torch.empty_like(e)
        _lib.check(_lib.load().fn_l2norm_fwd(_ptr(e), _ptr(embn), n, E, 1e-10, stream(self.device)), "l2norm_fwd")
        return e, embn, lab

    def loss(self, emb: torch.Tensor, labels, alpha: float = 0.2, soft: bool = False):
        """emb fp32 [N,E] un-normalised, labels [N].  -> (loss 0-d tensor, d loss / d emb [N,E], info dict, picks int32 [N,2]: the
        memory slot of each row's positive and negative pick, -1 where the pick is a batch row or the row is no anchor)."""
        lib, st = _lib.load(), stream(self.device)
        e, embn, lab = self._batch(emb, labels)
        n, E, M, dev = e.shape[0], self.E, self.size, self.device
        if n < 2:
            raise ValueError(f"the loss takes 2 to 1024 rows, got {n}")
        dist = torch.empty(n, n, dtype=torch.float32, device=dev)
        mem_dist = torch.empty(n, M, dtype=torch.float32, device=dev)
        _lib.check(lib.fn_pairwise_sqdist(_ptr(embn), _ptr(embn), _ptr(dist), None, n, n, E, 2, st), "pairwise_sqdist")
        _lib.check(lib.fn_pairwise_sqdist(_ptr(embn), _ptr(self.emb), _ptr(mem_dist), None, n, M, E, 2, st), "pairwise_sqdist")
        loss = torch.zeros(4, dtype=torch.float32, device=dev)
        coef = torch.empty(n, n, dtype=torch.float32, device=dev)
        mpick = torch.empty(n, 2, dtype=torch.int32, device=dev)
        mcoef = torch.empty(n, 2, dtype=torch.float32, device=dev)
        info = torch.zeros(8, dtype=torch.int32, device=dev)
        dembn, grad = torch.empty_like(e), torch.empty_like(e)
        _lib.check(lib.fn_xbm_triplet_fwd_bwd(_ptr(embn), _ptr(dist), _ptr(lab), _ptr(self.emb), _ptr(mem_dist), _ptr(self.labels),
                                              _ptr(self.state), _ptr(dembn), _ptr(loss), _ptr(coef), _ptr(mpick), _ptr(mcoef), _ptr(info),
                                              n, M, E, float(alpha), 1 if soft else 0, st), "xbm_triplet")
        _lib.check(lib.fn_l2norm_bwd(_ptr(e), _ptr(dembn), _ptr(grad), n, E, 1e-10, st), "l2norm_bwd")
        return loss[0], grad, memory_stats(info.cpu().tolist()), mpick

    def enqueue(self, emb: torch.Tensor, labels, start: int = 0):
        """Normalise emb [N,E] and write it with its labels behind the cursor (``start``: calls to let pass before the first row is
        stored)."""
        _, embn, lab = self._batch(emb, labels)
        _lib.check(_lib.load().fn_xbm_enqueue(_ptr(embn), _ptr(lab), _ptr(self.emb), _ptr(self.labels), _ptr(self.state), embn.shape[0],
                                              self.size, self.E, int(start), stream(self.device)), "xbm_enqueue")
