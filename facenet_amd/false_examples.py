"""False examples: WHICH pairs a threshold gets wrong, where ConfidenceMatrix and VerificationCurve count
them.  The reference's FalseExamples.write_false_pairs (facenet/statistics.py:334-421) with one launch of fn_false_pairs in place
of a NumPy distance matrix per pair of classes."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from ._call import check_int, check_unit_range, host_array, ptr, stream
from .utils import ConcatenateImages, file2text

MAX_PICKS = 64                   # fn_false_pairs: max_fneg and max_fpos
MAX_CLASS_ROWS = 65536           # the kernel's tie-break position is two 16-bit row numbers within the class
MAX_RECORDS = 1 << 20            # the default buffer's ceiling (16 MB)


def records_bound(sizes, max_fneg: int, max_fpos: int) -> int:
    """The most records a pool can yield: sum over classes of min(max_fneg, n // 2) plus sum over pairs of classes of
    min(max_fpos, n_a, n_b), the latter as sum over v <= max_fpos of the pairs of classes with at least v rows each."""
    sizes = np.asarray(sizes, dtype=np.int64)
    fneg = int(np.minimum(sizes // 2, max_fneg).sum())
    at_least = [int(np.count_nonzero(sizes >= v)) for v in range(1, max_fpos + 1)]
    return fneg + sum(c * (c - 1) // 2 for c in at_least)


class FalseExamples:
    """The worst pairs of a set of embeddings at a threshold, picked greedily as the reference does.  Per class the farthest
    pairs with d > threshold (false negatives, at most ``max_fneg``): a picked pair takes both its images out of the class's
    further picks.  Per pair of classes the nearest pairs with d < threshold (false positives, at most ``max_fpos``): a picked
    pair takes its image of the lower class and its image of the higher class out of that pair of classes' further picks.  Ties go
    to the pair that comes first in the row-major order of the reference's matrices (rows sorted by label, stable).  d is the
    distance ``ConfidenceMatrix``, ``VerificationCurve`` and ``Gallery`` compare, bit for bit, and the comparisons are theirs:
    strict fp32.  ``false_negatives`` / ``false_positives``: lists of (distance, index1, index2), indices into the caller's
    rows, in the order (class or pair of classes in label order, pick)."""

    def __init__(self, embeddings, labels, threshold, metric=0, files=None, max_fneg=10, max_fpos=2, device: str = "cuda",
                 atol: float = 1.e-5, max_records=None):
        from .statistics import SimilarityCalculator          # (statistics re-exports this module)
        if metric not in (0, 1):
            raise ValueError('Undefined similarity metric {}'.format(metric))
        self.metric, self.threshold = metric, float(np.float32(threshold))
        if np.isnan(self.threshold):
            raise ValueError("threshold must be a number, got NaN")
        self.max_fneg = check_int("max_fneg", max_fneg, 0, MAX_PICKS)
        self.max_fpos = check_int("max_fpos", max_fpos, 0, MAX_PICKS)
        labels = host_array(labels).reshape(-1)
        self.files = None if files is None else [str(f) for f in files]
        if self.files is not None and len(self.files) != len(labels):
            raise ValueError("files must name one file per label, got {} for {} labels".format(len(self.files), len(labels)))
        sizes = np.unique(labels, return_counts=True)[1]
        if len(labels) == 0:
            raise ValueError("false examples need at least one row")
        if sizes.max() > MAX_CLASS_ROWS:
            raise ValueError("a class has {} rows, more than the {} that false_pairs takes".format(int(sizes.max()), MAX_CLASS_ROWS))
        bound = records_bound(sizes, self.max_fneg, self.max_fpos)
        capacity = min(bound, MAX_RECORDS) if max_records is None else check_int("max_records", max_records, 0)

        calc = SimilarityCalculator(embeddings, labels, metric=metric, device=device)
        emb = calc.emb
        if emb.shape[1] % 4:       # zeros add fma(0, 0, acc) = acc: no bit of a dot product changes
            emb = torch.nn.functional.pad(emb, (0, 4 - emb.shape[1] % 4)).contiguous()
        order = np.argsort(labels, kind="stable")              # SimilarityCalculator's: sorted row -> the caller's row
        # one buffer, one fill, one download: count [2] uint64 | range [2] int32 and 8 spare bytes | records [capacity][4] int32
        buf = torch.empty(4 + 2 * capacity, dtype=torch.int64, device=emb.device)
        buf[:4].zero_()
        _lib.check(_lib.load().fn_false_pairs(ptr(emb), ptr(calc._cls), calc.nrof_classes, emb.shape[1], metric, self.threshold,
                                              self.max_fneg, self.max_fpos, ptr(buf, 4) if capacity else None, capacity, ptr(buf),
                                              ptr(buf, 2), stream(emb.device)), "false_pairs")
        host = buf.cpu()
        check_unit_range(host[2:3].view(torch.int32), atol)
        nneg, npos = (int(v) for v in host[:2])
        if nneg + npos > capacity:
            raise ValueError("false_pairs found {} pairs ({} false negatives, {} false positives), more than max_records = {}: "
                             "choose another threshold or a larger max_records".format(nneg + npos, nneg, npos, capacity))
        rec = host[4:].view(torch.int32).numpy().reshape(capacity, 4)
        cls = lambda rows: np.searchsorted(calc.class_start, rows, side="right") - 1
        self.false_negatives, self.false_positives = [], []
        for out, part in ((self.false_negatives, rec[:nneg]), (self.false_positives, rec[capacity - npos:])):
            part = part[np.lexsort((part[:, 3], cls(part[:, 1]), cls(part[:, 0])))]       # (class pair, pick): slots come in any order
            dist = np.ascontiguousarray(part[:, 2]).view(np.float32)
            out.extend((float(d), int(order[a]), int(order[b])) for d, a, b in zip(dist, part[:, 0], part[:, 1]))

    @property
    def nrof_false_negatives(self):
        return len(self.false_negatives)

    @property
    def nrof_false_positives(self):
        return len(self.false_positives)

    def _name(self, index):
        return str(index) if self.files is None else file2text(self.files[index])

    def __repr__(self):
        text = ('{}\nmetric: {}\nthreshold: {:2.5f}\n\nfalse negatives: {} (at most {} per class)\n'
                'false positives: {} (at most {} per pair of classes)\n').format(
                    self.__class__.__name__, self.metric, self.threshold, self.nrof_false_negatives, self.max_fneg,
                    self.nrof_false_positives, self.max_fpos)
        if self.false_negatives:
            d, a, b = max(self.false_negatives, key=lambda r: r[0])
            text += 'Farthest false negative: {:2.5f} {} & {}\n'.format(d, self._name(a), self._name(b))
        if self.false_positives:
            d, a, b = min(self.false_positives, key=lambda r: r[0])
            text += 'Nearest false positive: {:2.5f} {} & {}\n'.format(d, self._name(a), self._name(b))
        return text + '\n'

    def write_false_pairs(self, fpos_dir, fneg_dir):
        """One picture per pair (utils.ConcatenateImages) into the two directories, which are created."""
        from pathlib import Path
        if self.files is None:
            raise ValueError("write_false_pairs needs the files of the rows: FalseExamples(..., files=...)")
        for outdir, pairs in ((fpos_dir, self.false_positives), (fneg_dir, self.false_negatives)):
            outdir = Path(outdir).expanduser()
            outdir.mkdir(parents=True, exist_ok=True)
            for d, a, b in pairs:
                ConcatenateImages(self.files[a], self.files[b], d).save(outdir)


def false_examples(embeddings, labels, files, config, threshold, device: str = "cuda"):
    """The false examples ``config.false_examples`` asks for (a section with some of the keys threshold, max_fneg, max_fpos;
    ``threshold`` stands in when the section's own is null); None when the section is unset or empty: the one helper of
    apps/validate.py."""
    from .config import Config
    asked = getattr(config, "false_examples", None)
    if not asked:                                         # a Config reads a missing key as an empty Config
        return None
    asked = asked.as_dict if isinstance(asked, Config) else dict(asked)
    own = asked.get("threshold")
    picks = {k: asked[k] for k in ("max_fneg", "max_fpos") if asked.get(k) is not None}
    return FalseExamples(embeddings, labels, threshold if own is None else own, metric=config.metric, files=files, device=device, **picks)
