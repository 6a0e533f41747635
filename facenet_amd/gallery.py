"""The known faces on the device and every search over them (the map of the stack: `recognize.py`).  `Gallery._run` is the one
path from a set of queries to a launched fn_* search; ``search``, ``candidates``, ``mates`` and ``within``
are argument checks, one call of it and the shaping of its result, and `ivf.IVFGallery` overrides the launch of ``search`` alone."""
from __future__ import annotations

from pathlib import Path
from types import SimpleNamespace
from typing import NamedTuple

import numpy as np
import torch

from . import _lib
from ._call import as_table, check_int, check_unit_range, host_array, ptr, stream, workspace
from .faceclass import FaceToFaceNormalizedEmbeddingsClassifier
from .hierarchy import MAX_MIN_SAMPLES, SpanningTree

MAX_K = 64                # fn_gallery_search: 1 <= k <= 64
MAX_LENGTH = 512          # ... and embedding length a multiple of 4 up to 512
MAX_EDGES = 2 ** 31      # cols are int32 positions of a CSR that one allocation holds
DBSCAN_ROUNDS = 8         # rounds enqueued between two looks at the converged flag


def check_edges(nnz, max_edges=None):
    """The size rule of `Gallery.within`, applied before anything of that size is allocated."""
    if nnz >= MAX_EDGES:
        raise ValueError(f"the radius search found nnz = {nnz} neighbour pairs, 2^31 or more: choose a smaller eps")
    if max_edges is not None and nnz > max_edges:
        raise ValueError(f"the radius search found nnz = {nnz} neighbour pairs, more than max_edges = {max_edges}: choose a smaller eps")


def check_k(k):
    k = int(k)
    if not 1 <= k <= MAX_K:
        raise ValueError(f"k must be in [1, {MAX_K}], got {k}")
    return k


def shape_of(x):
    return tuple(x.shape) if hasattr(x, "shape") else np.shape(x)


def like_queries(queries, out):
    """NumPy in gives NumPy out, a device tensor in gives device tensors out (None stays None)."""
    if torch.is_tensor(queries):
        return out
    return tuple(None if t is None else t.cpu().numpy() for t in out)


class Clustering:
    """The result of `Gallery.cluster`: ``labels`` int64 [G] (cluster ids 0 .. nrof_clusters - 1 in ascending order of each
    cluster's smallest core row, -1 for noise), ``core`` bool [G], ``nrof_clusters``, ``nrof_noise``, ``rounds`` (hook-and-jump
    rounds run), ``eps`` / ``min_samples`` and the CSR it was built from: ``offsets`` int64 [G + 1], ``rows`` int32 [nnz],
    ``dist`` float32 [nnz] (device tensors)."""

    def __init__(self, labels, core, nrof_clusters, nrof_noise, rounds, eps, min_samples, offsets, rows, dist):
        self.labels, self.core = labels, core
        self.nrof_clusters, self.nrof_noise, self.rounds = nrof_clusters, nrof_noise, rounds
        self.eps, self.min_samples = eps, min_samples
        self.offsets, self.rows, self.dist = offsets, rows, dist

    @property
    def sizes(self):
        """int64 [nrof_clusters]: rows per cluster (noise rows are in none)."""
        return np.bincount(self.labels[self.labels >= 0], minlength=self.nrof_clusters).astype(np.int64)

    def members(self, c):
        """The rows of cluster c, ascending (c = -1: the noise rows)."""
        if not -1 <= c < self.nrof_clusters:
            raise ValueError(f"cluster {c} is not in [-1, {self.nrof_clusters})")
        return np.nonzero(self.labels == c)[0]

    def __repr__(self):
        return (f"{self.__class__.__name__}\n" + f"Number of images {len(self.labels)}\n" + f"Number of clusters {self.nrof_clusters}\n" +
                f"Number of noise images {self.nrof_noise}\n" + f"eps: {self.eps} min_samples: {self.min_samples}\n")


class MateSearch(NamedTuple):
    """What `Gallery.mates` returns, one entry per query row: the nearest mate's distance (float32) and gallery row (int32), the
    nearest impostor's, and ``ranks`` int32 (None when not asked for): the impostor rows nearer than the nearest mate.  Row -1,
    distance +inf and rank -1 where there is no such row."""
    mate_dist: object
    mate_rows: object
    impostor_dist: object
    impostor_rows: object
    ranks: object


def _class_names(labels, files):
    """label -> the name of the directory that holds one of its files (the class directories of dataset.Database)."""
    names = {}
    for label, f in zip(np.asarray(labels).tolist(), np.asarray(files).tolist()):
        names.setdefault(int(label), Path(str(f)).parent.name)
    return names


class Gallery:
    """The known faces: fp32 unit-norm embeddings [G, E] resident on the device, optionally an integer label per row (default:
    every row is its own class), a name per label (a dict, or a sequence indexed by label) and the file of every row.  ``metric``
    0 reports 2 (1 - x.y), 1 arccos(x.y) (statistics.py:45-53); both rank by the former.  Labels stay on the host as int64 and
    are looked up there from the rows a search returns (fn_gallery_search's own int32 ``labels`` table is not used), so any
    non-negative integer is a valid label."""

    def __init__(self, embeddings, labels=None, names=None, files=None, metric=0, device="cuda"):
        if metric not in (0, 1):
            raise ValueError("Undefined similarity metric {}".format(metric))            # statistics.py:55
        shape = shape_of(embeddings)
        if len(shape) != 2 or shape[0] < 1:
            raise ValueError(f"gallery embeddings must be a non-empty 2-D [G, E] array, got shape {shape}")
        if shape[1] % 4 or not 4 <= shape[1] <= MAX_LENGTH:
            raise ValueError(f"embedding length {shape[1]} must be a multiple of 4 in [4, {MAX_LENGTH}]")
        if labels is None:
            host_labels = np.arange(shape[0], dtype=np.int64)
        else:
            host_labels = host_array(labels)
            if host_labels.shape != (shape[0],) or host_labels.dtype.kind not in "iu":
                raise ValueError(f"labels must be {shape[0]} integers, got shape {host_labels.shape} of {host_labels.dtype}")
            if host_labels.min() < 0:
                raise ValueError("labels must not be negative: -1 is what an unidentified face gets")
        if files is not None and len(files) != shape[0]:
            raise ValueError(f"files must name {shape[0]} rows, got {len(files)}")
        if names is not None and not isinstance(names, dict):
            names = {i: n for i, n in enumerate(names)}
        if names is not None and not set(np.unique(host_labels).tolist()) <= set(names):
            raise ValueError("names must cover every label")
        self.metric, self.device = metric, torch.device(device)
        self.labels = host_labels.astype(np.int64)
        self.names = names
        self.files = None if files is None else np.asarray(files, dtype=str)
        self.embeddings = as_table(embeddings, self.device)
        self._codes = None         # `_label_codes`

    @classmethod
    def from_file(cls, path, metric=0, device="cuda"):
        """The .npz of apps/embeddings.py (``embeddings`` / ``labels`` / ``files``); names are the class directories of ``files``."""
        path = Path(path).expanduser()
        if path.suffix == ".h5":
            raise ValueError(f"{path}: .h5 embeddings files need h5py, which this project does not use; "
                             "write an .npz with 'embeddings' and 'labels' (facenet_amd.apps.embeddings)")
        with np.load(path) as f:
            embeddings = np.asarray(f["embeddings"], dtype=np.float32)
            labels = np.asarray(f["labels"]) if "labels" in f else None
            files = np.asarray(f["files"]) if "files" in f else None
        names = _class_names(labels, files) if labels is not None and files is not None else None
        return cls(embeddings, labels=labels, names=names, files=files, metric=metric, device=device)

    @property
    def nrof_images(self):
        return self.embeddings.shape[0]

    @property
    def nrof_classes(self):
        return len(np.unique(self.labels))

    @property
    def length(self):
        return self.embeddings.shape[1]

    def __repr__(self):
        return (f"{self.__class__.__name__}\n" + f"Number of classes {self.nrof_classes} \n" + f"Number of images {self.nrof_images}\n" +
                f"Embedding length {self.length}\n" + f"metric: {self.metric}\n")

    def _run(self, runs, queries, skip, atol, outputs, sizer, size, launch, then=None):
        """From the queries of a search to its device outputs: check the queries and ``skip``, allocate ``outputs(Q)``, and for
        Q = 0 return them as they are: nothing needs a device or the library.  Otherwise (``runs`` names the method and its entry
        for the error on a host gallery) upload both, size the workspace with fn_<sizer>(*size(Q)), zero the two `range` words
        unless ``atol`` is None, call ``launch(c, *outputs)``, which makes and checks the ctypes call, and check the range, which
        waits for the search.  ``c`` holds ``lib``, ``Q``, the device tables ``queries`` (fp32 [Q, E]) and ``skip`` (int32 [Q] or
        None), ``workspace``, ``range`` (None without a check) and ``stream``.  ``then(c, *outputs)`` -> outputs: a second pass
        that needs the first one's results on the host."""
        shape = shape_of(queries)
        if len(shape) != 2:
            raise ValueError(f"queries must be a 2-D [Q, E] array, got shape {shape}")
        if shape[1] != self.length:
            raise ValueError(f"embedding lengths differ: queries {shape[1]}, gallery {self.length}")
        Q, dev = shape[0], self.device
        if skip is not None:
            skip = host_array(skip)
            if skip.shape != (Q,) or skip.dtype.kind not in "iu":
                raise ValueError(f"skip must be {Q} integers (a gallery row, or -1), got shape {skip.shape} of {skip.dtype}")
        out = outputs(Q)
        if Q == 0:
            return out
        if dev.type != "cuda":
            raise _lib.FacenetHipError(f"{runs} on the GPU; facenet_amd has no CPU fallback")
        lib = _lib.load()
        c = SimpleNamespace(lib=lib, Q=Q, queries=as_table(queries, dev), stream=stream(dev),
                            skip=None if skip is None else torch.from_numpy(skip.astype(np.int32)).to(dev),
                            workspace=workspace(dev, getattr(lib, "fn_" + sizer), sizer, *size(Q)),
                            range=None if atol is None else torch.zeros(2, dtype=torch.int32, device=dev))
        launch(c, *out)
        if c.range is not None:
            check_unit_range(c.range, atol)         # waits for the search
        return out if then is None else then(c, *out)

    def _nearest(self, Q, k):
        """The outputs of a k-nearest search: (dist float32 [Q, k], rows int32 [Q, k])."""
        return torch.empty((Q, k), dtype=torch.float32, device=self.device), torch.empty((Q, k), dtype=torch.int32, device=self.device)

    def _search(self, queries, k, skip=None, slab_rows=0, atol=1.e-5):
        """-> device (dist [Q, k], rows [Q, k]) after every check of `search`: the launch `search` and `identify` go through."""
        k, G, slab_rows = check_k(k), self.nrof_images, int(slab_rows)

        def launch(c, dist, rows):
            _lib.check(c.lib.fn_gallery_search(ptr(c.queries), c.Q, ptr(self.embeddings), G, self.length, k, self.metric, ptr(c.skip), None,
                                               slab_rows, ptr(c.workspace), ptr(dist), ptr(rows), None, ptr(c.range), c.stream), "gallery_search")

        return self._run("Gallery.search runs fn_gallery_search", queries, skip, atol, lambda Q: self._nearest(Q, k),
                         "gallery_search_workspace", lambda Q: (Q, G, k, slab_rows), launch)

    def search(self, queries, k=1, skip=None, slab_rows=0, atol=1.e-5):
        """The k nearest gallery rows of every query row -> (dist float32 [Q, k], rows int32 [Q, k]), ascending by (distance,
        row); NumPy in gives NumPy out, a device tensor in gives device tensors out.  ``skip`` [Q]: the gallery row query q must
        not return (-1: none).  A query with fewer than k admissible rows gets row -1 at distance +inf in the tail.  Raises the
        reference's ValueError when some dot product leaves +-(1 + atol); that check reads two words back and so waits for the
        search on the host, also when tensors go in and come out.  ``atol=None`` leaves the check out: the call then only
        enqueues work on the current stream.  ``slab_rows`` is fn_gallery_search's (0: chosen by the library; the result does not
        depend on it)."""
        return like_queries(queries, self._search(queries, k, skip, slab_rows, atol))

    def leave_one_out(self, k=1):
        """Every gallery row's k nearest OTHER rows, device tensors: ``search(gallery, k, skip=arange(G))``."""
        return self.search(self.embeddings, k, skip=np.arange(self.nrof_images, dtype=np.int32))

    def _candidates(self, queries, k, skip=None, slab_rows=0, atol=1.e-5):
        """-> device (dist [Q, k], rows [Q, k]) after every check of `candidates`: the launch of fn_gallery_candidates."""
        k, G, slab_rows = check_k(k), self.nrof_images, int(slab_rows)

        def launch(c, dist, rows):
            _lib.check(c.lib.fn_gallery_candidates(ptr(c.queries), c.Q, ptr(self.embeddings), G, ptr(self._label_codes()[1]), self.length, k,
                                                   self.metric, ptr(c.skip), slab_rows, ptr(c.workspace), ptr(dist), ptr(rows), ptr(c.range),
                                                   c.stream), "gallery_candidates")

        return self._run("Gallery.candidates runs fn_gallery_candidates", queries, skip, atol, lambda Q: self._nearest(Q, k),
                         "gallery_candidates_workspace", lambda Q: (Q, G, k, slab_rows), launch)

    def candidates(self, queries, k=1, skip=None, slab_rows=0, atol=1.e-5):
        """The candidate list of every query row: its k nearest IDENTITIES (distinct labels), each through its nearest gallery row
         -> (dist float32 [Q, k], rows int32 [Q, k], labels int64 [Q, k]), ascending by (distance, row);
        NumPy in gives NumPy out, a device tensor in gives device tensors out.  ``rows[q, j]`` is the nearest row of the j-th
        identity (equal distances go to the lower row), ``dist`` its distance, `search`'s bit for bit, and ``labels`` its label,
        looked up on the host from the rows.  Column 0 is `search`'s.  A query with fewer than k admissible identities gets row
        -1, distance +inf and label -1 in the tail.  ``k`` in [1, 64] counts identities however many rows each has, which
        `search` cannot promise at any k.  ``skip``, ``slab_rows``, ``atol`` and the ValueError for unnormalised embeddings: as
        `search`.  ``statistics.cmc(labels, rows)`` of these rows is the identity-level cumulative match curve: a mate at column
        j has j impostor identities in front of it, not j impostor rows."""
        dist, rows = self._candidates(queries, k, skip, slab_rows, atol)
        found = rows.cpu().numpy()
        labels = np.where(found >= 0, self.labels[np.maximum(found, 0)], -1).astype(np.int64)
        if torch.is_tensor(queries):
            return dist, rows, torch.from_numpy(labels).to(rows.device)
        return dist.cpu().numpy(), found, labels

    def leave_one_out_candidates(self, k=1):
        """Every gallery row's k nearest identities among all OTHER rows, device tensors: ``candidates(gallery, k,
        skip=arange(G))``.  A probe's own identity is a candidate whenever it has another row, so ``statistics.cmc(labels,
        rows)`` of the rows returned is the identity-level cumulative match curve of the gallery."""
        return self.candidates(self.embeddings, k, skip=np.arange(self.nrof_images, dtype=np.int32))

    def identify_candidates(self, queries, k, threshold=None, classifier=None):
        """-> for every query row the list of (label, name, distance, row) of its candidates (`candidates`, `who`), nearest first:
        at most k distinct identities.  Open set (``threshold`` or ``classifier``, as `identify`): the list stops at the first
        candidate that fails ``distance < threshold`` (strict, fp32), so it may be empty.  Closed set: every identity found."""
        thr = self.threshold_of(threshold, classifier)
        dist, rows = (t.cpu().numpy() for t in self._candidates(queries, k))
        out = []
        for d, r in zip(dist, rows):
            n = int((r >= 0).sum())                            # (the tail is behind every candidate)
            if thr is not None:
                n = min(n, int(np.argmin(np.append(d[:n] < thr, False))))
            out.append([self.who(d[j], r[j], thr) for j in range(n)])
        return out

    def templates(self):
        """One template per identity -> a new `Gallery` with one row per label, in ascending label order: the L2-normalised mean
        of that label's rows, from one launch of fn_kmeans_update (sequential fp64 sums in ascending row order, one rounding to
        fp32: reproducible bit for bit).  Its labels are the sorted unique labels, so its searches answer in identities; names
        and the metric carry over, ``files`` is None.  Raises a ValueError naming the label when a label's rows sum to zero: such
        an identity has no direction."""
        dev, E = self.device, self.length
        if dev.type != "cuda":
            raise _lib.FacenetHipError("Gallery.templates runs fn_kmeans_update on the GPU; facenet_amd has no CPU fallback")
        uniq = self._label_codes()[0]
        codes = np.searchsorted(uniq, self.labels)
        order = torch.from_numpy(np.argsort(codes, kind="stable").astype(np.int32)).to(dev)          # by (label, row)
        list_start = torch.from_numpy(np.concatenate([[0], np.cumsum(np.bincount(codes, minlength=len(uniq)))]).astype(np.int32)).to(dev)
        prev = torch.zeros((len(uniq), E), dtype=torch.float32, device=dev)
        means = torch.empty_like(prev)
        kept = torch.empty(len(uniq), dtype=torch.int32, device=dev)
        _lib.check(_lib.load().fn_kmeans_update(ptr(self.embeddings), self.nrof_images, E, ptr(order), ptr(list_start), len(uniq), ptr(prev), ptr(means), ptr(kept), stream(dev)), "kmeans_update")
        flat = np.nonzero(kept.cpu().numpy())[0]
        if len(flat):
            raise ValueError(f"the rows of label {int(uniq[flat[0]])} sum to zero: that identity has no template")
        return Gallery(means, labels=uniq, names=self.names, metric=self.metric, device=dev)

    def kmeans(self, nlist, iters=10, seed=0):
        """Spherical k-means of the gallery's rows into ``nlist`` groups on the device -> (centroids fp32
        [nlist, E], assign int32 [G], info): `ivf.kmeans`.  Reproducible bit for bit for a given seed."""
        from .ivf import kmeans             # ivf.py subclasses Gallery: it imports this module
        return kmeans(self, nlist, iters, seed)

    def ivf(self, nlist, iters=10, seed=0):
        """The inverted-file index of this gallery over the k-means of its rows -> `ivf.IVFGallery`, whose searches walk only
        the lists a query probes."""
        from .ivf import ivf
        return ivf(self, nlist, iters, seed)

    def quantize(self, shortlist=64):
        """This gallery with int8 codes of its rows -> `quantized.QuantizedGallery`, whose searches take a
        shortlist of ``shortlist`` rows on the int8 MFMA, rank it exactly and fall back to `search` where that is not provably
        the exhaustive answer."""
        from .quantized import quantize
        return quantize(self, shortlist)

    def _label_codes(self):
        """(the gallery's sorted unique labels int64 [C], device int32 [G] dense codes 0 .. C - 1), built once: fn_mate_search
        compares int32 codes, whatever non-negative int64 the labels are."""
        if self._codes is None:
            uniq, inverse = np.unique(self.labels, return_inverse=True)
            codes = torch.from_numpy(inverse.reshape(-1).astype(np.int32))
            self._codes = (uniq, codes.to(self.device) if self.device.type == "cuda" else codes)
        return self._codes

    def query_codes(self, labels, Q):
        """Query labels -> int32 [Q] codes of the gallery's table: -1 for -1 and for a label the gallery does not hold."""
        labels = host_array(labels)
        if labels.shape != (Q,) or (Q and labels.dtype.kind not in "iu"):        # (an empty list has no integer type)
            raise ValueError(f"labels must be {Q} integers (the probe's identity, or -1), got shape {labels.shape} of {labels.dtype}")
        labels = labels.astype(np.int64)
        if Q and labels.min() < -1:
            raise ValueError("a query label must not be below -1: -1 is a probe known to be absent from the gallery")
        uniq = self._label_codes()[0]
        at = np.minimum(np.searchsorted(uniq, labels), len(uniq) - 1)
        return np.where(uniq[at] == labels, at, -1).astype(np.int32)

    def mates(self, queries, labels, skip=None, ranks=True, slab_rows=0, atol=1.e-5):
        """The open-set evaluation search: for every query row its nearest MATE (the nearest gallery row
        that carries the query's label) and its nearest IMPOSTOR (the nearest row of any other label) -> `MateSearch`; NumPy in
        gives NumPy out, a device tensor in gives device tensors out.  ``labels`` [Q]: the probes' identities in the gallery's
        own labels; -1, or a label the gallery does not hold, is a probe without a mate: every row is its impostor.  ``ranks``:
        also the number of impostor rows nearer than the nearest mate (-1 without a mate), the 0-based rank of the first mate in
        the full ordering, at any depth; it costs a second walk of the gallery.  Where there is no such row: row -1, distance
        +inf.  Equal distances go to the lower row; the distances are `search`'s bit for bit.  ``skip``, ``slab_rows``,
        ``atol``: as `search`."""
        shape = shape_of(queries)
        if len(shape) == 2 and shape[1] == self.length:        # (else `_run` raises)
            codes = self.query_codes(labels, shape[0])         # before anything needs a device
        dev, G, slab_rows = self.device, self.nrof_images, int(slab_rows)

        def outputs(Q):
            return (torch.empty((Q, 2), dtype=torch.float32, device=dev), torch.empty((Q, 2), dtype=torch.int32, device=dev),
                    torch.empty(Q, dtype=torch.int32, device=dev) if ranks else None)

        def launch(c, dist, rows, rank):
            qcodes = torch.from_numpy(codes).to(dev)
            _lib.check(c.lib.fn_mate_search(ptr(c.queries), c.Q, ptr(qcodes), ptr(self.embeddings), G, ptr(self._label_codes()[1]), self.length,
                                            self.metric, ptr(c.skip), slab_rows, ptr(c.workspace), ptr(dist), ptr(rows), ptr(rank), ptr(c.range),
                                            c.stream), "mate_search")

        dist, rows, rank = self._run("Gallery.mates runs fn_mate_search", queries, skip, atol, outputs, "mate_search_workspace",
                                     lambda Q: (Q, G, slab_rows), launch)
        return MateSearch(*like_queries(queries, (dist[:, 0], rows[:, 0], dist[:, 1], rows[:, 1], rank)))

    def leave_one_out_mates(self, ranks=True):
        """Every gallery row as a probe against all OTHER rows, device tensors: ``mates(gallery, labels, skip=arange(G))``."""
        return self.mates(self.embeddings, self.labels, skip=np.arange(self.nrof_images, dtype=np.int32), ranks=ranks)

    def threshold_of(self, threshold=None, classifier=None):
        """The fp32 threshold of `identify`: the number given, a classifier's trained one, or None (closed set)."""
        if threshold is not None and classifier is not None:
            raise ValueError("identify takes a threshold or a classifier, not both")
        if classifier is not None:
            if not isinstance(classifier, FaceToFaceNormalizedEmbeddingsClassifier):
                raise ValueError("identify needs a FaceToFaceNormalizedEmbeddingsClassifier: its distance is the gallery's metric 0")
            if self.metric != 0:
                raise ValueError("a classifier's threshold applies to metric 0, this gallery reports metric {}".format(self.metric))
            return classifier.variable("threshold", mode="numpy")
        return None if threshold is None else np.float32(threshold)

    def identify(self, queries, threshold=None, classifier=None, k=1, **index):
        """-> for every query row (label, name, distance, row) of its nearest gallery row.  ``k`` is the width of the search that
        is run; only its best column is used, so any k gives the same answer and k = 1 is the cheapest.  Open set:
        label -1 and name None unless ``distance < threshold`` (the strict < of the classifiers' predict, in fp32); the
        threshold is the number given or ``classifier.variable("threshold")``.  Neither: closed set, always the nearest.
        ``**index``: the keywords of an index's own search (`ivf.IVFGallery`: ``nprobe``); a plain gallery takes none."""
        thr = self.threshold_of(threshold, classifier)
        dist, rows = self._search(queries, k, **index)
        return [self.who(d, r, thr) for d, r in zip(dist[:, 0].cpu().numpy(), rows[:, 0].cpu().numpy())]

    def who(self, distance, row, threshold=None):
        """(label, name, distance, row) of one search result: label -1, name None when there is no row or, with an fp32
        ``threshold`` (`threshold_of`), ``distance < threshold`` is false."""
        known = row >= 0 and (threshold is None or distance < threshold)
        label = int(self.labels[row]) if known else -1
        return label, (self.names[label] if known and self.names is not None else None), float(distance), int(row)

    def within(self, queries, eps, skip=None, slab_rows=0, atol=1.e-5, max_edges=None):
        """Every gallery row at ``distance < eps`` (the gallery's metric, strict fp32 <) of every query row, as a CSR ->
        (offsets int64 [Q + 1], rows int32 [nnz], dist float32 [nnz]): query q's neighbours are rows[offsets[q]:offsets[q + 1]],
        ascending by gallery row.  NumPy in gives NumPy out, a device tensor in gives device tensors out.  ``skip`` [Q]: the
        gallery row query q must not return (-1: none).  The call reads nnz back between its two passes, so it waits for the
        device.  Raises the reference's ValueError when some dot product leaves +-(1 + atol) (``atol=None``: no such check), and a
        ValueError naming nnz when it exceeds ``max_edges`` or reaches 2^31, before the rows are allocated.  ``slab_rows`` is
        fn_radius_count's (0: chosen by the library; the result does not depend on it)."""
        eps = np.float32(eps)
        if np.isnan(eps):
            raise ValueError("eps must be a number, got NaN")
        if max_edges is not None and max_edges < 0:
            raise ValueError(f"max_edges must not be negative, got {max_edges}")
        dev, G, slab_rows = self.device, self.nrof_images, int(slab_rows)

        def outputs(Q):
            return (torch.zeros(Q + 1, dtype=torch.int64, device=dev), torch.empty(0, dtype=torch.int32, device=dev),
                    torch.empty(0, dtype=torch.float32, device=dev))

        def common(c):
            return (ptr(c.queries), c.Q, ptr(self.embeddings), G, self.length, self.metric, float(eps), ptr(c.skip), slab_rows, ptr(c.workspace))

        def count(c, offsets, rows, dist):
            _lib.check(c.lib.fn_radius_count(*common(c), ptr(offsets), ptr(c.range), c.stream), "radius_count")

        def fill(c, offsets, rows, dist):
            nnz = int(offsets[c.Q].item())                              # waits for the count
            check_edges(nnz, max_edges)
            rows = torch.empty(nnz, dtype=torch.int32, device=dev)
            dist = torch.empty(nnz, dtype=torch.float32, device=dev)
            if nnz:
                _lib.check(c.lib.fn_radius_fill(*common(c), ptr(rows), ptr(dist), nnz, c.stream), "radius_fill")
            return offsets, rows, dist

        return like_queries(queries, self._run("Gallery.within runs fn_radius_count", queries, skip, atol, outputs, "radius_workspace",
                                               lambda Q: (Q, G, slab_rows), count, then=fill))

    def neighbours(self, eps, max_edges=None):
        """The self-join, device tensors: every gallery row's OTHER rows within eps, ``within(gallery, eps, skip=arange(G))``.
        The distances are symmetric bit for bit, so row j is in i's list exactly when i is in j's."""
        return self.within(self.embeddings, eps, skip=np.arange(self.nrof_images, dtype=np.int32), max_edges=max_edges)

    def cluster(self, threshold=None, classifier=None, min_samples=1, max_edges=None):
        """DBSCAN over the gallery's rows at eps = the threshold (a number, or a trained classifier's: `threshold_of`) -> a
        `Clustering`.  A row is a core row when it has at least ``min_samples`` rows within eps, itself included; clusters are
        the connected components of the core rows; a non-core row with a core neighbour joins its nearest core neighbour's
        cluster (equal distances: the lower row); every other row is noise, label -1.  ``min_samples=1`` is single linkage at
        the threshold."""
        if threshold is None and classifier is None:
            raise ValueError("cluster needs a threshold or a classifier: clustering has no closed set")
        min_samples = check_int("min_samples", min_samples, 1)
        eps = self.threshold_of(threshold, classifier)
        offsets, rows, dist = self.neighbours(eps, max_edges=max_edges)
        dev, N = self.device, self.nrof_images
        lib = _lib.load()
        labels = torch.empty(N, dtype=torch.int32, device=dev)
        core = torch.empty(N, dtype=torch.int32, device=dev)
        ids = torch.empty(N, dtype=torch.int32, device=dev)
        info = torch.zeros(8, dtype=torch.int32, device=dev)
        st = stream(dev)
        _lib.check(lib.fn_dbscan_init(N, ptr(offsets), min_samples, ptr(labels), ptr(core), ptr(info), st), "dbscan_init")
        while True:
            _lib.check(lib.fn_dbscan_rounds(N, ptr(offsets), ptr(rows), ptr(core), ptr(labels), ptr(info), DBSCAN_ROUNDS, st), "dbscan_rounds")
            if int(info[0].item()):
                break
        _lib.check(lib.fn_dbscan_finish(N, ptr(offsets), ptr(rows), ptr(dist), self.metric, ptr(self.embeddings), self.length, ptr(core),
                                        ptr(labels), ptr(ids), ptr(info), st), "dbscan_finish")
        _, rounds, clusters, noise = info.cpu().tolist()[:4]
        return Clustering(labels.cpu().numpy().astype(np.int64), core.cpu().numpy().astype(bool), clusters, noise, rounds, float(eps),
                          min_samples, offsets, rows, dist)

    def spanning_tree(self, min_samples=1, slab_rows=0):
        """The minimum spanning tree of the gallery's rows under the mutual-reachability distance w(i, j) = max(d(i, j), core[i],
        core[j]) -> `hierarchy.SpanningTree`, built on the device by Boruvka's algorithm (fn_mst_*): at
        most ceil(log2 N) walks of all pairs, and the [N, N] matrix never reaches memory.  ``core[i]`` is the distance to the
        (min_samples - 1)-th nearest OTHER row (`leave_one_out`, the same bits), 0 for ``min_samples=1``, which makes the tree
        single linkage's.  The tree is the unique one under the edge order (bits(w), lo, hi): it depends neither on ``slab_rows``
        (fn_mst_rounds', 0: chosen by the library) nor on scheduling.  Metric 0 only."""
        N = self.nrof_images
        min_samples = check_int("min_samples", min_samples, 1, min(MAX_MIN_SAMPLES, N), note=" (at most the number of rows)")
        if self.metric != 0:
            raise ValueError("a spanning tree needs metric 0, whose distances are pinned bit for bit; this gallery reports metric {}".format(self.metric))
        dev, slab_rows = self.device, int(slab_rows)
        if dev.type != "cuda":
            raise _lib.FacenetHipError("Gallery.spanning_tree runs fn_mst_rounds on the GPU; facenet_amd has no CPU fallback")
        core = None
        if min_samples > 1:
            core = self.leave_one_out(min_samples - 1)[0][:, min_samples - 2].contiguous()
        lib, st = _lib.load(), stream(dev)
        work = workspace(dev, lib.fn_mst_workspace, "mst_workspace", N, slab_rows)
        comp = torch.empty(N, dtype=torch.int32, device=dev)
        edges = torch.empty((max(N - 1, 1), 2), dtype=torch.int32, device=dev)
        weights = torch.empty(max(N - 1, 1), dtype=torch.float32, device=dev)
        info = torch.zeros(8, dtype=torch.int32, device=dev)
        _lib.check(lib.fn_mst_init(N, ptr(comp), ptr(info), st), "mst_init")
        rounds = max(1, int(N - 1).bit_length())               # ceil(log2 N): Boruvka's bound
        _lib.check(lib.fn_mst_rounds(ptr(self.embeddings), N, self.length, ptr(core), slab_rows, ptr(work), ptr(comp), ptr(edges), ptr(weights),
                                     ptr(info), rounds, st), "mst_rounds")
        done, ran, components, written = info.cpu().tolist()[:4]
        if not done or written != N - 1:
            raise _lib.FacenetHipError(f"fn_mst_rounds left {components} components after {ran} rounds: are the embeddings numbers?")
        host_core = np.zeros(N, dtype=np.float32) if core is None else core.cpu().numpy()
        return SpanningTree.from_edges(edges[:N - 1].cpu().numpy(), weights[:N - 1].cpu().numpy(), host_core, rounds=ran, min_samples=min_samples)

    def hdbscan(self, min_cluster_size=5, min_samples=None, method="eom", allow_single_cluster=False, slab_rows=0):
        """HDBSCAN over the gallery's rows, no threshold at all -> `hierarchy.HierarchicalClustering`:
        ``spanning_tree(min_samples).hdbscan(min_cluster_size, method, allow_single_cluster)``.  ``min_samples=None`` means
        ``min_cluster_size``, as scikit-learn does."""
        check_int("min_cluster_size", min_cluster_size, 2)
        if method not in ("eom", "leaf"):
            raise ValueError(f"method must be 'eom' or 'leaf', got {method!r}")
        tree = self.spanning_tree(min_cluster_size if min_samples is None else min_samples, slab_rows=slab_rows)
        return tree.hdbscan(min_cluster_size, method=method, allow_single_cluster=allow_single_cluster)
