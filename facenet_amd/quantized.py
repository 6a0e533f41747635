"""The quantised gallery: an int8 shortlist, the exact fp32 re-rank of it and a certificate.

``Gallery.quantize()`` -> `QuantizedGallery`, which keeps the fp32 table (the re-rank, the fallback and the inherited ``mates`` /
``within`` / ``cluster`` need it) and adds what fn_quantize_rows gives for it: ``codes`` int8 [G, Ep], ``scale`` / ``rho`` /
``norm`` fp32 [G] and the maxima ``rho_max`` / ``norm_max``.  ``search`` quantises the queries, takes each query's ``shortlist``
nearest rows by the int8 dot product (fn_qgallery_search, v_mfma_i32_16x16x64_i8), ranks those by `Gallery.search`'s own fp32 key
and proves per query whether a row outside the shortlist could have entered the top k.  ``exact=True`` (the default) runs the
queries without that proof through `Gallery._search` and scatters them in: the result is `Gallery.search`'s bit for bit on every
input, and the quantisation only decides how many queries pay for the fallback (``last_fallbacks``).  ``exact=False`` returns the
re-ranked shortlist as it is."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from ._call import as_table, check_int, host_array, ptr, stream
from .gallery import Gallery, check_k, like_queries

PAD = 64                  # code rows are padded to a multiple of this
MAX_SHORTLIST = 64        # fn_qgallery_search: k <= shortlist <= 64


def padded_length(E):
    return (E + PAD - 1) // PAD * PAD


def check_shortlist(shortlist, k):
    return check_int("shortlist", shortlist, k, MAX_SHORTLIST, note=" (k to 64 rows)")


def quantize_rows(rows):
    """fp32 [N, E] on the device -> (codes int8 [N, Ep], scale, rho, norm fp32 [N]): one fn_quantize_rows call, enqueued."""
    N, E = rows.shape
    dev = rows.device
    codes = torch.empty((N, padded_length(E)), dtype=torch.int8, device=dev)
    scale, rho, norm = (torch.empty(N, dtype=torch.float32, device=dev) for _ in range(3))
    _lib.check(_lib.load().fn_quantize_rows(ptr(rows), N, E, ptr(codes), ptr(scale), ptr(rho), ptr(norm), stream(dev)), "quantize_rows")
    return codes, scale, rho, norm


class QuantizedGallery(Gallery):
    """A `Gallery` whose ``search``, ``leave_one_out`` and ``identify`` go through the int8 shortlist.  ``shortlist`` is the
    default of the searches (64); ``last_fallbacks`` the number of queries the last ``exact=True`` search ran again."""

    def __init__(self, embeddings, labels=None, names=None, files=None, metric=0, device="cuda", shortlist=MAX_SHORTLIST):
        super().__init__(embeddings, labels=labels, names=names, files=files, metric=metric, device=device)
        self.shortlist = check_int("shortlist", shortlist, 1, MAX_SHORTLIST)
        self.codes = self.scale = self.rho = self.norm = self.rho_max = self.norm_max = None
        if self.device.type == "cuda":                        # (a host gallery checks arguments and raises at its first search)
            self.codes, self.scale, self.rho, self.norm = quantize_rows(self.embeddings)
            self.rho_max, self.norm_max = float(self.rho.max().item()), float(self.norm.max().item())
        self.last_fallbacks = 0

    def __repr__(self):
        return super().__repr__() + f"int8 codes, shortlist: {self.shortlist}\n"

    def _certified_search(self, queries, k, skip, slab_rows, atol, shortlist):
        """-> device (dist [Q, k], rows [Q, k], certified int32 [Q]) of one fn_qgallery_search call."""
        k = check_k(k)
        R = check_shortlist(max(self.shortlist, k) if shortlist is None else shortlist, k)
        G, E, slab_rows, dev = self.nrof_images, self.length, int(slab_rows), self.device

        def outputs(Q):
            return self._nearest(Q, k) + (torch.empty(Q, dtype=torch.int32, device=dev),)

        def launch(c, dist, rows, certified):
            codes, scale, rho, norm = quantize_rows(c.queries)
            _lib.check(c.lib.fn_qgallery_search(ptr(c.queries), c.Q, ptr(self.embeddings), G, ptr(codes), ptr(scale), ptr(self.codes),
                                                ptr(self.scale), ptr(rho), ptr(norm), self.rho_max, self.norm_max, E, k, R, self.metric,
                                                ptr(c.skip), slab_rows, ptr(c.workspace), ptr(dist), ptr(rows), ptr(certified), None,
                                                ptr(c.range), c.stream), "qgallery_search")

        return self._run("QuantizedGallery.search runs fn_qgallery_search", queries, skip, atol, outputs, "qgallery_search_workspace",
                         lambda Q: (Q, G, k, R, slab_rows), launch)

    def _search(self, queries, k, skip=None, slab_rows=0, atol=1.e-5, *, shortlist=None, exact=True):
        """-> device (dist [Q, k], rows [Q, k]) after every check of `search`."""
        if not isinstance(exact, (bool, np.bool_)):
            raise ValueError(f"exact must be True or False, got {exact!r}")
        dist, rows, certified = self._certified_search(queries, k, skip, slab_rows, atol, shortlist)
        if not exact or dist.shape[0] == 0:
            return dist, rows
        again = torch.nonzero(certified == 0).view(-1)         # reads certified back: waits for the search
        self.last_fallbacks = int(again.numel())
        if self.last_fallbacks:
            sub_skip = None if skip is None else host_array(skip)[again.cpu().numpy()]
            d2, r2 = Gallery._search(self, as_table(queries, self.device)[again], k, sub_skip, slab_rows, atol)
            dist.index_copy_(0, again, d2)
            rows.index_copy_(0, again, r2)
        return dist, rows

    def search(self, queries, k=1, skip=None, slab_rows=0, atol=1.e-5, shortlist=None, exact=True):
        """`Gallery.search` through the int8 shortlist of ``shortlist`` rows (k <= shortlist <= 64; None: the gallery's default,
        at least k): the same return types and errors.  ``exact=True``: the queries the certificate does not cover are run again
        through the exhaustive search, so the result is `Gallery.search`'s bit for bit; the call reads the certificate back and so
        waits for the device.  ``exact=False``: the re-ranked shortlist as it is: every distance is exact for its row, but a nearer
        row may be missing; with ``atol=None`` the call only enqueues.  The normalisation check covers the pairs re-ranked (and,
        for a query run again, all of its pairs), not all Q x G pairs."""
        return like_queries(queries, self._search(queries, k, skip, slab_rows, atol, shortlist=shortlist, exact=exact))

    def search_certified(self, queries, k=1, skip=None, slab_rows=0, atol=1.e-5, shortlist=None):
        """The re-ranked shortlist with its certificate -> (dist, rows, certified bool [Q]); no fallback is run.  Where
        ``certified`` holds, that query's dist and rows are `Gallery.search`'s bit for bit."""
        dist, rows, certified = self._certified_search(queries, k, skip, slab_rows, atol, shortlist)
        return like_queries(queries, (dist, rows, certified != 0))

    def leave_one_out(self, k=1, shortlist=None, exact=True):
        """Every gallery row's k nearest OTHER rows, device tensors."""
        return self.search(self.embeddings, k, skip=np.arange(self.nrof_images, dtype=np.int32), shortlist=shortlist, exact=exact)

    def quantize(self, shortlist=None):
        return self if shortlist is None else quantize(self, shortlist)


def quantize(gallery, shortlist=MAX_SHORTLIST):
    """`Gallery.quantize`: the quantised gallery over the same fp32 table, labels, names, files and metric."""
    from .ivf import IVFGallery
    if isinstance(gallery, IVFGallery):
        raise NotImplementedError("quantised inverted-file lists are not built: quantize the Gallery the index was built from")
    shortlist = check_int("shortlist", shortlist, 1, MAX_SHORTLIST)
    return QuantizedGallery(gallery.embeddings, labels=gallery.labels, names=gallery.names, files=gallery.files, metric=gallery.metric,
                            device=gallery.device, shortlist=shortlist)
