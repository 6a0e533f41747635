"""The inverted-file (IVF) index of a gallery: spherical k-means on the device and an exact search over
the lists a query probes.

``kmeans(gallery, nlist, iters, seed)`` (reached as ``Gallery.kmeans``): the centroids start as the rows at the first ``nlist``
positions of ``np.random.RandomState(seed).permutation(G)``; an iteration assigns every row to its nearest centroid with
fn_gallery_search (k = 1: ascending (d0, centroid index), exact), sorts the rows by (list, row) and runs fn_kmeans_update.  It
stops early when no assignment changed.  Every step is reproducible bit for bit, so the same seed gives the same index.

``IVFGallery`` stores the gallery's rows list by list with ``ids`` (the original row of each stored row, ascending within a
list), ``list_start`` and the centroids as a small `Gallery`.  ``search`` takes each query's ``nprobe`` nearest centroids as
its probes and runs fn_ivf_search: the distances, the order and the row numbers are `Gallery.search`'s, restricted to the rows
of the probed lists.  The only approximation is which lists get probed; with ``nprobe == nlist`` the answer is the exhaustive
one bit for bit."""
from __future__ import annotations

from pathlib import Path

import numpy as np
import torch

from . import _lib
from .faceclass import _ptr, _stream
from .recognize import MAX_K, Gallery
from .statistics import check_unit_range


def check_nlist(nlist, G):
    if isinstance(nlist, bool) or not isinstance(nlist, (int, np.integer)) or not 1 <= nlist <= G:
        raise ValueError(f"nlist must be an integer in [1, {G}] (the gallery's rows), got {nlist!r}")
    return int(nlist)


def check_nprobe(nprobe):
    if isinstance(nprobe, bool) or not isinstance(nprobe, (int, np.integer)) or nprobe < 1:
        raise ValueError(f"nprobe must be an integer of at least 1, got {nprobe!r}")
    return int(nprobe)


def initial_rows(G, nlist, seed):
    """The rows the centroids start from."""
    return np.random.RandomState(seed).permutation(G)[:nlist]


def kmeans(gallery, nlist, iters=10, seed=0):
    """-> (centroids fp32 [nlist, E], assign int32 [G], info), device tensors.  ``assign`` is every row's nearest centroid among
    the ones returned.  ``info``: ``iterations`` (centroid updates run), ``moved`` (rows whose list changed at each assignment
    step; the first counts every row), ``empty`` (lists without a row in ``assign``) and ``converged``."""
    G = gallery.nrof_images
    nlist = check_nlist(nlist, G)
    if isinstance(iters, bool) or not isinstance(iters, (int, np.integer)) or iters < 0:
        raise ValueError(f"iters must be a non-negative integer, got {iters!r}")
    dev, E = gallery.device, gallery.length
    if dev.type != "cuda":
        raise _lib.FacenetHipError("Gallery.kmeans runs fn_kmeans_update on the GPU; facenet_amd has no CPU fallback")
    lib, rows, st = _lib.load(), gallery.embeddings, _stream(dev)
    centroids = rows[torch.from_numpy(initial_rows(G, nlist, seed)).to(dev)].contiguous()
    ws = gallery._workspace(lib.fn_gallery_search_workspace, "gallery_search_workspace", G, nlist, 1, 0)
    dist = torch.empty((G, 1), dtype=torch.float32, device=dev)
    kept = torch.empty(nlist, dtype=torch.int32, device=dev)

    def assign_step():
        near = torch.empty((G, 1), dtype=torch.int32, device=dev)
        _lib.check(lib.fn_gallery_search(_ptr(rows), G, _ptr(centroids), nlist, E, 1, 0, None, None, 0, _ptr(ws), _ptr(dist), _ptr(near), None,
                                         None, st), "gallery_search")
        return near.view(G)

    assign, moved, updates, converged = None, [], 0, False
    for _ in range(iters):
        new = assign_step()
        moved.append(G if assign is None else int((new != assign).sum().item()))
        assign = new
        if moved[-1] == 0:
            converged = True
            break
        order = torch.sort(assign, stable=True)[1].to(torch.int32)           # by (list, row): the sort is stable
        list_start = torch.zeros(nlist + 1, dtype=torch.int32, device=dev)
        list_start[1:] = torch.cumsum(torch.bincount(assign, minlength=nlist), 0)
        updated = torch.empty_like(centroids)
        _lib.check(lib.fn_kmeans_update(_ptr(rows), G, E, _ptr(order), _ptr(list_start), nlist, _ptr(centroids), _ptr(updated), _ptr(kept), st),
                   "kmeans_update")
        centroids, updates = updated, updates + 1
    if not converged:                                                        # the rows' lists under the centroids returned
        new = assign_step()
        moved.append(G if assign is None else int((new != assign).sum().item()))
        assign, converged = new, moved[-1] == 0
    empty = int((torch.bincount(assign, minlength=nlist) == 0).sum().item())
    return centroids, assign, {"iterations": updates, "moved": moved, "empty": empty, "converged": converged}


def _host(x):
    return np.asarray(x.cpu() if torch.is_tensor(x) else x)


class IVFGallery(Gallery):
    """A `Gallery` whose ``search``, ``leave_one_out`` and ``identify`` walk only the ``nprobe`` lists nearest to each query.
    Labels, names, files and the metric are the parent's, and every row number that goes in (``skip``) or comes out is a row of
    the parent gallery.  ``lists`` fp32 [G, E] (device), ``ids`` / ``list_start`` (host int32, and on the device), ``centroids``
    a `Gallery` of the nlist centroids, ``nprobe`` the default of the searches (8).  ``labels`` and ``files`` are indexed by
    ORIGINAL row, as in the parent."""

    def __init__(self, lists, ids, list_start, centroids, labels=None, names=None, files=None, metric=0, device="cuda", nprobe=8):
        super().__init__(lists, labels=labels, names=names, files=files, metric=metric, device=device)
        G = self.nrof_images
        ids, list_start = _host(ids), _host(list_start)
        if ids.shape != (G,) or ids.dtype.kind not in "iu" or not np.array_equal(np.sort(ids), np.arange(G)):
            raise ValueError(f"ids must be a permutation of the {G} gallery rows")
        if list_start.ndim != 1 or len(list_start) < 2 or list_start.dtype.kind not in "iu" or list_start[0] != 0 or list_start[-1] != G \
                or (np.diff(list_start) < 0).any():
            raise ValueError(f"list_start must ascend from 0 to {G}")
        starts = np.zeros(G, dtype=bool)
        starts[list_start[:-1][list_start[:-1] < G]] = True
        if G > 1 and not (starts[1:] | (np.diff(ids) > 0)).all():
            raise ValueError("ids must ascend within every list")
        self.ids, self.list_start = ids.astype(np.int32), list_start.astype(np.int32)
        if not isinstance(centroids, Gallery):
            centroids = Gallery(centroids, metric=metric, device=device)
        if centroids.nrof_images != self.nlist or centroids.length != self.length:
            raise ValueError(f"centroids must be [{self.nlist}, {self.length}], got [{centroids.nrof_images}, {centroids.length}]")
        self.centroids, self.nprobe = centroids, check_nprobe(nprobe)
        self._ids_dev = self._list_start_dev = None

    @property
    def lists(self):
        return self.embeddings

    @property
    def nlist(self):
        return len(self.list_start) - 1

    @classmethod
    def from_assignment(cls, gallery, centroids, assign, nprobe=8):
        """The index of ``gallery`` under any assignment of its rows to lists: ``centroids`` [nlist, E], ``assign`` [G] integers
        in [0, nlist).  Rows keep their order within a list."""
        G, E = gallery.nrof_images, gallery.length
        shape = tuple(centroids.shape) if hasattr(centroids, "shape") else np.shape(centroids)
        if len(shape) != 2 or shape[0] < 1 or shape[1] != E:
            raise ValueError(f"centroids must be a non-empty 2-D [nlist, {E}] array, got shape {shape}")
        assign = _host(assign)
        if assign.shape != (G,) or assign.dtype.kind not in "iu":
            raise ValueError(f"assign must be {G} integers (the list of every row), got shape {assign.shape} of {assign.dtype}")
        if G and (assign.min() < 0 or assign.max() >= shape[0]):
            raise ValueError(f"assign must name lists in [0, {shape[0]}), got [{assign.min()}, {assign.max()}]")
        ids = np.argsort(assign, kind="stable").astype(np.int32)
        list_start = np.concatenate([[0], np.cumsum(np.bincount(assign, minlength=shape[0]))]).astype(np.int32)
        lists = gallery.embeddings[torch.from_numpy(ids.astype(np.int64)).to(gallery.device)]
        return cls(lists, ids, list_start, centroids, labels=gallery.labels, names=gallery.names, files=gallery.files, metric=gallery.metric,
                   device=gallery.device, nprobe=nprobe)

    def save(self, path):
        """One .npz: the stored rows, ``ids``, ``list_start``, the centroids, and the labels / names / files by original row."""
        path = Path(path).expanduser()
        if path.suffix != ".npz":
            raise ValueError(f"{path}: an index is saved as an .npz")
        extra = {}
        if self.files is not None:
            extra["files"] = self.files
        if self.names is not None:
            keys = sorted(self.names)
            extra.update(name_labels=np.asarray(keys, dtype=np.int64), name_values=np.asarray([str(self.names[c]) for c in keys], dtype=str))
        np.savez(path, lists=self.embeddings.cpu().numpy(), ids=self.ids, list_start=self.list_start,
                 centroids=self.centroids.embeddings.cpu().numpy(), labels=self.labels, metric=np.int64(self.metric),
                 nprobe=np.int64(self.nprobe), **extra)
        return path

    @classmethod
    def load(cls, path, device="cuda"):
        with np.load(Path(path).expanduser()) as f:
            names = dict(zip(f["name_labels"].tolist(), f["name_values"].tolist())) if "name_labels" in f else None
            return cls(f["lists"], f["ids"], f["list_start"], f["centroids"], labels=f["labels"], names=names,
                       files=f["files"] if "files" in f else None, metric=int(f["metric"]), device=device, nprobe=int(f["nprobe"]))

    def __repr__(self):
        return super().__repr__() + f"Number of lists {self.nlist} nprobe: {self.nprobe}\n"

    def _index(self):
        if self._ids_dev is None:
            self._ids_dev = torch.from_numpy(self.ids).to(self.device)
            self._list_start_dev = torch.from_numpy(self.list_start).to(self.device)
        return self._ids_dev, self._list_start_dev

    def _search(self, queries, k, skip, slab_rows, atol, nprobe=None):
        """-> device (dist [Q, k], rows [Q, k]) after every check of `search`."""
        k = int(k)
        if not 1 <= k <= MAX_K:
            raise ValueError(f"k must be in [1, {MAX_K}], got {k}")
        nprobe = min(check_nprobe(self.nprobe if nprobe is None else nprobe), self.nlist)
        if nprobe > MAX_K:
            raise ValueError(f"nprobe must be at most {MAX_K} (the centroid search keeps k <= {MAX_K}), got {nprobe}")
        Q, q, skip_dev = self._queries(queries, skip, "IVFGallery.search runs fn_ivf_search")
        dev, G, L = self.device, self.nrof_images, self.nlist
        dist = torch.empty((Q, k), dtype=torch.float32, device=dev)
        rows = torch.empty((Q, k), dtype=torch.int32, device=dev)
        if Q == 0:
            return dist, rows
        lib = _lib.load()
        probes = self.centroids._search(q, nprobe, None, 0, None)[1]
        ids, list_start = self._index()
        ws = self._workspace(lib.fn_ivf_search_workspace, "ivf_search_workspace", Q, L, nprobe, self.length, k)
        rng = None if atol is None else torch.zeros(2, dtype=torch.int32, device=dev)
        _lib.check(lib.fn_ivf_search(_ptr(q), Q, _ptr(self.embeddings), _ptr(ids), G, _ptr(list_start), L, self.length, _ptr(probes), nprobe, k,
                                     self.metric, _ptr(skip_dev), _ptr(ws), _ptr(dist), _ptr(rows), _ptr(rng), _stream(dev)), "ivf_search")
        if rng is not None:
            check_unit_range(rng, atol)         # waits for the search
        return dist, rows

    def search(self, queries, k=1, nprobe=None, skip=None, atol=1.e-5):
        """`Gallery.search` over the ``nprobe`` lists nearest to each query (None: the index's default; clamped to nlist):
        the same return types, the same errors, rows and ``skip`` in the parent gallery's row numbers.  A query whose lists hold
        fewer than k admissible rows gets row -1 at distance +inf in the tail.  The normalisation check covers the pairs
        evaluated."""
        dist, rows = self._search(queries, k, skip, 0, atol, nprobe)
        if torch.is_tensor(queries):
            return dist, rows
        return dist.cpu().numpy(), rows.cpu().numpy()

    def leave_one_out(self, k=1, nprobe=None):
        """Every gallery row's k nearest OTHER rows among its probed lists, device tensors indexed by ORIGINAL row."""
        dist, rows = self.search(self.embeddings, k, nprobe=nprobe, skip=self.ids)
        ids = self._index()[0].long()
        return torch.empty_like(dist).index_copy_(0, ids, dist), torch.empty_like(rows).index_copy_(0, ids, rows)

    def identify(self, queries, threshold=None, classifier=None, k=1, nprobe=None):
        """`Gallery.identify` through the probed lists."""
        thr = self.threshold_of(threshold, classifier)
        dist, rows = self._search(queries, k, None, 0, 1.e-5, nprobe)
        return [self.who(d, r, thr) for d, r in zip(dist[:, 0].cpu().numpy(), rows[:, 0].cpu().numpy())]

    def _not_indexed(self, *args, **kwargs):
        raise NotImplementedError("an IVFGallery answers search, leave_one_out and identify; run this on the Gallery it was built from")

    mates = leave_one_out_mates = within = neighbours = cluster = kmeans = ivf = _not_indexed


def ivf(gallery, nlist, iters=10, seed=0, nprobe=8):
    """k-means, then the index of its assignment -> `IVFGallery` (``kmeans_info``: what `kmeans` reported)."""
    centroids, assign, info = kmeans(gallery, nlist, iters, seed)
    index = IVFGallery.from_assignment(gallery, centroids, assign, nprobe=nprobe)
    index.kmeans_info = info
    return index
