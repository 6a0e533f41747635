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
from ._call import check_int, host_array, ptr, stream
from .gallery import MAX_K, Gallery, check_k, like_queries, shape_of


def initial_rows(G, nlist, seed):
    """The rows the centroids start from."""
    return np.random.RandomState(seed).permutation(G)[:nlist]


def kmeans(gallery, nlist, iters=10, seed=0):
    """-> (centroids fp32 [nlist, E], assign int32 [G], info), device tensors.  ``assign`` is every row's nearest centroid among
    the ones returned.  ``info``: ``iterations`` (centroid updates run), ``moved`` (rows whose list changed at each assignment
    step; the first counts every row), ``empty`` (lists without a row in ``assign``) and ``converged``."""
    G = gallery.nrof_images
    nlist = check_int("nlist", nlist, 1, G, note=" (the gallery's rows)")
    iters = check_int("iters", iters, 0)
    dev, E = gallery.device, gallery.length
    if dev.type != "cuda":
        raise _lib.FacenetHipError("Gallery.kmeans runs fn_kmeans_update on the GPU; facenet_amd has no CPU fallback")
    lib, rows, st = _lib.load(), gallery.embeddings, stream(dev)
    centroids = rows[torch.from_numpy(initial_rows(G, nlist, seed)).to(dev)].contiguous()
    kept = torch.empty(nlist, dtype=torch.int32, device=dev)

    def assign_step(assign):
        """Every row's nearest centroid: the rows as the queries of a search over the centroids (metric 0, no range check)."""
        new = Gallery(centroids, device=dev)._search(rows, 1, atol=None)[1].view(G)
        moved.append(G if assign is None else int((new != assign).sum().item()))
        return new

    assign, moved, updates, converged = None, [], 0, False
    for _ in range(iters):
        assign = assign_step(assign)
        if moved[-1] == 0:
            converged = True
            break
        order = torch.sort(assign, stable=True)[1].to(torch.int32)           # by (list, row): the sort is stable
        list_start = torch.zeros(nlist + 1, dtype=torch.int32, device=dev)
        list_start[1:] = torch.cumsum(torch.bincount(assign, minlength=nlist), 0)
        updated = torch.empty_like(centroids)
        _lib.check(lib.fn_kmeans_update(ptr(rows), G, E, ptr(order), ptr(list_start), nlist, ptr(centroids), ptr(updated), ptr(kept), st),
                   "kmeans_update")
        centroids, updates = updated, updates + 1
    if not converged:                                                        # the rows' lists under the centroids returned
        assign = assign_step(assign)
        converged = moved[-1] == 0
    empty = int((torch.bincount(assign, minlength=nlist) == 0).sum().item())
    return centroids, assign, {"iterations": updates, "moved": moved, "empty": empty, "converged": converged}


class IVFGallery(Gallery):
    """A `Gallery` whose ``search``, ``leave_one_out`` and ``identify`` walk only the ``nprobe`` lists nearest to each query.
    Labels, names, files and the metric are the parent's, and every row number that goes in (``skip``) or comes out is a row of
    the parent gallery.  ``lists`` fp32 [G, E] (device), ``ids`` / ``list_start`` (host int32, and on the device), ``centroids``
    a `Gallery` of the nlist centroids, ``nprobe`` the default of the searches (8).  ``labels`` and ``files`` are indexed by
    ORIGINAL row, as in the parent."""

    def __init__(self, lists, ids, list_start, centroids, labels=None, names=None, files=None, metric=0, device="cuda", nprobe=8):
        super().__init__(lists, labels=labels, names=names, files=files, metric=metric, device=device)
        G = self.nrof_images
        ids, list_start = host_array(ids), host_array(list_start)
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
        self.centroids, self.nprobe = centroids, check_int("nprobe", nprobe, 1)
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
        shape = shape_of(centroids)
        if len(shape) != 2 or shape[0] < 1 or shape[1] != E:
            raise ValueError(f"centroids must be a non-empty 2-D [nlist, {E}] array, got shape {shape}")
        assign = host_array(assign)
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

    def _search(self, queries, k, skip=None, slab_rows=0, atol=1.e-5, *, nprobe=None):
        """-> device (dist [Q, k], rows [Q, k]) after every check of `search`.  ``slab_rows`` has no meaning here."""
        k = check_k(k)
        nprobe = min(check_int("nprobe", self.nprobe if nprobe is None else nprobe, 1), self.nlist)
        if nprobe > MAX_K:
            raise ValueError(f"nprobe must be at most {MAX_K} (the centroid search keeps k <= {MAX_K}), got {nprobe}")
        G, L = self.nrof_images, self.nlist

        def launch(c, dist, rows):
            probes = self.centroids._search(c.queries, nprobe, atol=None)[1]
            ids, list_start = self._index()
            _lib.check(c.lib.fn_ivf_search(ptr(c.queries), c.Q, ptr(self.embeddings), ptr(ids), G, ptr(list_start), L, self.length, ptr(probes),
                                           nprobe, k, self.metric, ptr(c.skip), ptr(c.workspace), ptr(dist), ptr(rows), ptr(c.range), c.stream),
                       "ivf_search")

        return self._run("IVFGallery.search runs fn_ivf_search", queries, skip, atol, lambda Q: self._nearest(Q, k), "ivf_search_workspace",
                         lambda Q: (Q, L, nprobe, self.length, k), launch)

    def search(self, queries, k=1, nprobe=None, skip=None, atol=1.e-5):
        """`Gallery.search` over the ``nprobe`` lists nearest to each query (None: the index's default; clamped to nlist):
        the same return types, the same errors, rows and ``skip`` in the parent gallery's row numbers.  A query whose lists hold
        fewer than k admissible rows gets row -1 at distance +inf in the tail.  The normalisation check covers the pairs
        evaluated."""
        return like_queries(queries, self._search(queries, k, skip, atol=atol, nprobe=nprobe))

    def leave_one_out(self, k=1, nprobe=None):
        """Every gallery row's k nearest OTHER rows among its probed lists, device tensors indexed by ORIGINAL row."""
        dist, rows = self.search(self.embeddings, k, nprobe=nprobe, skip=self.ids)
        ids = self._index()[0].long()
        return torch.empty_like(dist).index_copy_(0, ids, dist), torch.empty_like(rows).index_copy_(0, ids, rows)

    def _not_indexed(self, *args, **kwargs):
        raise NotImplementedError("an IVFGallery answers search, leave_one_out and identify; run this on the Gallery it was built from")

    mates = leave_one_out_mates = within = neighbours = cluster = kmeans = ivf = _not_indexed
    candidates = leave_one_out_candidates = identify_candidates = templates = _not_indexed      # (they walk the rows in gallery order)


def ivf(gallery, nlist, iters=10, seed=0, nprobe=8):
    """k-means, then the index of its assignment -> `IVFGallery` (``kmeans_info``: what `kmeans` reported)."""
    centroids, assign, info = kmeans(gallery, nlist, iters, seed)
    index = IVFGallery.from_assignment(gallery, centroids, assign, nprobe=nprobe)
    index.kmeans_info = info
    return index
