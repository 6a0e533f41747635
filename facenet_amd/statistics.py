"""``pairwise_similarities`` with the reference's signature and error behaviour (facenet/statistics.py:22-57),
computed by the wavefront-reduced fn_pairwise_sqdist kernel."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from ._call import _decode_ord, check_int, check_unit_range, host_array, ptr, stream      # noqa: F401  (the tests read _decode_ord here)
from .gallery import Gallery


def pairwise_similarities(xa, xb=None, metric: int = 0, atol: float = 1.e-5, device: str = "cuda"):
    """xa [n,E], xb [m,E] unit-norm rows -> 2(1 - xa.xb^T) (metric 0) or arccos (metric 1); with ``xb=None`` the strict
    upper triangle of xa against itself, flattened row-major (np.triu_indices order)."""
    lib = _lib.load()
    if metric not in (0, 1):
        raise ValueError("Undefined similarity metric {}".format(metric))      # statistics.py:55
    a = torch.as_tensor(np.asarray(xa) if not torch.is_tensor(xa) else xa).to(device=device, dtype=torch.float32).contiguous()
    b = a if xb is None else torch.as_tensor(np.asarray(xb) if not torch.is_tensor(xb) else xb).to(device=device, dtype=torch.float32).contiguous()
    n, m, E = a.shape[0], b.shape[0], a.shape[1]
    if n == 0 or m == 0:
        return np.zeros((0,) if xb is None else (n, m), dtype=np.float32)
    out = torch.empty(n, m, dtype=torch.float32, device=a.device)
    rng = torch.zeros(2, dtype=torch.int32, device=a.device)
    _lib.check(lib.fn_pairwise_sqdist(ptr(a), ptr(b), ptr(out), ptr(rng), n, m, E, metric, stream(a.device)), "pairwise_sqdist")
    if xb is None:
        iu = torch.triu_indices(n, n, offset=1, device=a.device)
        sims = out[iu[0], iu[1]]
        if sims.numel() == 0:
            return sims.cpu().numpy()
    else:
        sims = out
    check_unit_range(rng, atol)         # the kernel reports min/max over the full matrix
    return sims.cpu().numpy()


def cmc(labels, rows):
    """Closed-set cumulative match curve of a leave-one-out search (host NumPy).  labels [n]: the class of every gallery row;
    rows int [n, k]: row i's neighbours in ascending distance, itself excluded, -1 where there is none (Gallery.leave_one_out).
    -> (curve float64 [k], left_out): curve[r] is the share of rows whose first r + 1 neighbours contain their own label.  A
    row whose class has no other image cannot be matched: such rows are left out of the share and counted in left_out."""
    labels, rows = np.asarray(labels), np.asarray(rows)
    if rows.ndim != 2 or rows.shape[0] != labels.shape[0]:
        raise ValueError("cmc: rows must be [len(labels), k], got {} for {} labels".format(rows.shape, labels.shape[0]))
    _, inverse, counts = np.unique(labels, return_inverse=True, return_counts=True)
    scored = counts[inverse] > 1
    left_out = int(np.count_nonzero(~scored))
    if not scored.any():
        return np.zeros(rows.shape[1], dtype=np.float64), left_out
    hit = (labels[np.maximum(rows, 0)] == labels[:, None]) & (rows >= 0)
    found = np.logical_or.accumulate(hit[scored], axis=1)
    return found.mean(axis=0, dtype=np.float64), left_out


def pairwise_clustering_scores(truth, labels):
    """Pairwise (precision, recall, F) of a clustering against the true classes, the usual face-clustering measure: of all
    pairs of rows that share a cluster the share that share a class, of all pairs that share a class the share that share a
    cluster, and their harmonic mean.  ``labels`` < 0 are noise rows: each is a cluster of its own.  Computed from the
    contingency table in exact (Python) integers; a ratio with an empty denominator is 1, as in ConfidenceMatrix."""
    truth, labels = np.asarray(truth), np.asarray(labels)
    if truth.ndim != 1 or truth.shape != labels.shape:
        raise ValueError("pairwise_clustering_scores: truth and labels must be 1-D and of equal length, got {} and {}".format(
            truth.shape, labels.shape))
    if labels.dtype.kind not in "iu":
        raise ValueError("pairwise_clustering_scores: labels must be integers, got {}".format(labels.dtype))
    n = len(labels)
    _, t = np.unique(truth, return_inverse=True)
    labels = labels.astype(np.int64)
    noise = labels < 0
    c = np.where(noise, (labels.max() + 1 if n else 0) + np.arange(n), labels)        # every noise row a singleton
    _, c = np.unique(c, return_inverse=True)
    pairs = lambda counts: sum(int(k) * (int(k) - 1) // 2 for k in counts)
    nt = int(t.max()) + 1 if n else 1
    _, cell = np.unique(c.astype(np.int64) * nt + t, return_counts=True)                # the non-empty cells of the table
    both, same_cluster, same_class = pairs(cell), pairs(np.bincount(c)), pairs(np.bincount(t))
    precision = both / same_cluster if same_cluster else 1.0
    recall = both / same_class if same_class else 1.0
    f = 2 * precision * recall / (precision + recall) if precision + recall else 0.0
    return precision, recall, f


# ------------------------------------------------------------------------------------------------------------------
# Face-to-face validation (facenet/statistics.py:82-331) on the GPU.  Same class names, properties and report text as
# the reference; the O(classes^2 x thresholds) NumPy loops run as ONE launch of fn_confidence_counts per matrix.
# ------------------------------------------------------------------------------------------------------------------
class SimilarityCalculator:
    """statistics.py:82-108.  Holds the embeddings grouped by class on the device (rows sorted by label)."""

    def __init__(self, embeddings, labels, metric=0, device: str = "cuda"):
        self.metric = metric
        labels = np.asarray(labels)
        emb = embeddings if torch.is_tensor(embeddings) else torch.as_tensor(np.asarray(embeddings))
        order = np.argsort(labels, kind="stable")
        uniq, counts = np.unique(labels, return_counts=True)
        self.class_start = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
        self.emb = emb.to(device=device, dtype=torch.float32)[torch.as_tensor(order, device=device)].contiguous()
        self._cls = torch.as_tensor(self.class_start, device=self.emb.device)

    @property
    def nrof_classes(self):
        return len(self.class_start) - 1

    def nrof_images(self, i):
        return int(self.class_start[i + 1] - self.class_start[i])

    def evaluate(self, i, k):
        """statistics.py:92-103 for one class pair (host convenience; ConfidenceMatrix does not loop over it)."""
        a = self.emb[self.class_start[i]:self.class_start[i + 1]]
        if i == k:
            sims = pairwise_similarities(a, None, self.metric, device=str(self.emb.device))
            weight = sims.size * self.nrof_classes
        else:
            b = self.emb[self.class_start[k]:self.class_start[k + 1]]
            sims = pairwise_similarities(a, b, self.metric, device=str(self.emb.device))
            weight = sims.size * (self.nrof_classes * (self.nrof_classes - 1) / 2)
        return sims, weight


def _ratio_or_one(num, den):
    """num / den element-wise, 1 where den == 0 (an empty positive or negative set scores perfectly, statistics.py:144-168)."""
    num, den = np.asarray(num, dtype=np.float64), np.asarray(den, dtype=np.float64)
    return np.divide(num, den, out=np.ones_like(den), where=den > 0)


def _ascending_f32(thresholds):
    """The thresholds as the count kernels take them: fp32 [T], ascending (their binning is a search over them)."""
    thr = np.array(thresholds, ndmin=1).astype(np.float32)
    if thr.size > 1 and not np.all(np.diff(thr) >= 0):
        raise ValueError("thresholds must be ascending")
    return thr


class ConfidenceMatrix:
    """Interface of statistics.py:111-175 (attributes tp / tn / fp / fn / threshold, the six rate properties).  The
    class-balanced counts for ALL thresholds come from one fn_confidence_counts launch into ``counts`` [4, T]; every rate is
    a ratio of two rows of it."""

    _ROWS = {"tp": 0, "tn": 1, "fp": 2, "fn": 3}

    def __init__(self, calculator: SimilarityCalculator, threshold, atol: float = 1.e-5):
        lib = _lib.load()
        self.threshold = np.array(threshold, ndmin=1)
        thr = _ascending_f32(self.threshold)
        dev = calculator.emb.device
        t_dev = torch.as_tensor(thr, device=dev)
        out = torch.zeros(4 * thr.size, dtype=torch.float64, device=dev)
        rng = torch.zeros(2, dtype=torch.int32, device=dev)
        n, E = calculator.emb.shape
        _lib.check(lib.fn_confidence_counts(ptr(calculator.emb), ptr(calculator._cls), calculator.nrof_classes, E, ptr(t_dev), thr.size,
                                            calculator.metric, ptr(out), ptr(rng), stream(dev)), "confidence_counts")
        self.counts = out.cpu().numpy().reshape(4, thr.size)
        check_unit_range(rng, atol)

    @classmethod
    def from_counts(cls, counts, threshold):
        """A matrix over an existing [4, T] table (rows tp / tn / fp / fn), e.g. one fold of fn_confidence_counts_folds."""
        self = cls.__new__(cls)
        self.threshold = np.array(threshold, ndmin=1)
        self.counts = np.asarray(counts, dtype=np.float64).reshape(4, self.threshold.size)
        return self

    def __getattr__(self, name):        # tp, tn, fp, fn are views of the count table
        row = ConfidenceMatrix._ROWS.get(name)
        if row is None or "counts" not in self.__dict__:
            raise AttributeError(name)
        return self.counts[row]

    @property
    def accuracy(self):
        return (self.tp + self.tn) / self.counts.sum(axis=0)

    @property
    def precision(self):
        return _ratio_or_one(self.tp, self.tp + self.fp)

    @property
    def tp_rates(self):      # sensitivity / recall
        return _ratio_or_one(self.tp, self.tp + self.fn)

    @property
    def tn_rates(self):      # specificity
        return _ratio_or_one(self.tn, self.tn + self.fp)

    @property
    def fp_rates(self):      # false alarm rate
        return 1 - self.tn_rates

    @property
    def fn_rates(self):
        return 1 - self.tp_rates


def far_threshold_slinear(fp_rates, thresholds, far_target):
    """statistics.py:299-302 ``interp1d(fp_rates, thresholds, kind='slinear')(far_target)``; fp_rates repeats values, which
    the scipy the reference ran accepted and current scipy rejects: piecewise-linear between the LAST threshold whose
    fp_rate <= far_target and the FIRST one above it."""
    fp = np.asarray(fp_rates, dtype=np.float64)
    thr = np.asarray(thresholds, dtype=np.float64)
    j = int(np.searchsorted(fp, far_target, side="right")) - 1
    if j < 0:
        return thr[0]
    if j >= len(fp) - 1:
        return thr[-1]
    if fp[j + 1] == fp[j]:
        return thr[j]
    return thr[j] + (far_target - fp[j]) / (fp[j + 1] - fp[j]) * (thr[j + 1] - thr[j])


_SCORED = ("accuracy", "precision", "tp_rates", "tn_rates", "threshold")     # keys of Report.dict besides auc / eer
_REPORT_LINES = (("Accuracy:  ", "accuracy"), ("Precision: ", "precision"), ("Sensitivity (TPR, 1-a type 1 error): ", "tp_rates"),
                 ("Specificity (TNR, 1-b type 2 error): ", "tn_rates"), ("Threshold: ", "threshold"))


def _roc_summary(fpr, tpr):
    """(AUC, EER) of a ROC polyline; -1 where the reference's try/except leaves its default (statistics.py:212-222)."""
    import sklearn.metrics
    from scipy import interpolate
    from scipy.optimize import brentq
    auc = eer = -1
    try:
        auc = sklearn.metrics.auc(fpr, tpr)
    except Exception:
        pass
    try:
        roc = interpolate.interp1d(fpr, tpr)
        eer = brentq(lambda x: 1. - x - roc(x), 0., 1.)
    except Exception:
        pass
    return auc, eer


class Report:
    """Interface of statistics.py:178-234 (criterion, conf_matrix_train / conf_matrix_test, append_fold, dict, the report
    text).  The dictionary is computed from stacked [folds, ...] arrays; the text is rendered from a line table."""

    def __init__(self, criterion=None):
        self.criterion = criterion
        self.conf_matrix_train = []
        self.conf_matrix_test = []

    def append_fold(self, name, conf_matrix):
        (self.conf_matrix_train if name == 'train' else self.conf_matrix_test).append(conf_matrix)

    @property
    def dict(self):
        train = self.conf_matrix_train
        tpr = np.stack([m.tp_rates for m in train]).mean(axis=0)
        fpr = 1 - np.stack([m.tn_rates for m in train]).mean(axis=0)
        auc, eer = _roc_summary(fpr, tpr)
        out = {'auc': auc, 'eer': eer}
        for key in _SCORED:
            per_fold = np.array([getattr(m, key) for m in self.conf_matrix_test])
            out[key] = per_fold.mean()
            out[key + '_std'] = per_fold.std()
        return out

    def __repr__(self):
        d = self.dict
        head = '{}\nArea under curve (AUC): {:1.5f}\nEqual error rate (EER): {:1.5f}\n\n'.format(self.criterion, d['auc'], d['eer'])
        # the reference prints std(precision_std) -- the spread of a scalar, i.e. 0 -- on the precision line (statistics.py:196)
        spread = {k: (0.0 if k == 'precision' else d[k + '_std']) for _, k in _REPORT_LINES}
        body = ''.join('{}{:2.5f}+-{:2.5f}\n'.format(label, d[k], spread[k]) for label, k in _REPORT_LINES)
        return head + body + '\n'


ONE_PASS_MAX_FOLDS = 16            # fn_confidence_counts_folds: 2 <= folds <= 16, thresholds <= 256
ONE_PASS_MAX_THRESHOLDS = 256


def kfold_assignment(nrof_images: int, nrof_folds: int):
    """(fold [n]: the fold of KFold(nrof_folds, shuffle=True, random_state=0) each image index is held out in, the list of
    (train, test) index arrays of that split)."""
    from sklearn.model_selection import KFold
    splits = list(KFold(n_splits=nrof_folds, shuffle=True, random_state=0).split(np.arange(nrof_images)))
    fold = np.empty(nrof_images, dtype=np.int32)
    for f, (_, test_set) in enumerate(splits):
        fold[test_set] = f
    return fold, splits


def fold_tables(labels, fold, nrof_folds: int):
    """Host tables of fn_confidence_counts_folds for rows sorted by label (stable): (order, class_start [C+1], fold of the
    sorted rows [n], train_rows [C, F] = rows of class c not held out in fold f, train_classes [F] = classes with such a row)."""
    labels, fold = np.asarray(labels), np.asarray(fold)
    if fold.shape != labels.shape or (fold.size and (fold.min() < 0 or fold.max() >= nrof_folds)):
        raise ValueError("fold must hold one index in [0, {}) per label".format(nrof_folds))
    order = np.argsort(labels, kind="stable")
    _, cls, counts = np.unique(labels[order], return_inverse=True, return_counts=True)
    held_out = np.zeros((len(counts), nrof_folds), dtype=np.int64)
    np.add.at(held_out, (cls, fold[order]), 1)
    train_rows = counts[:, None] - held_out
    class_start = np.concatenate([[0], np.cumsum(counts)])
    return (order, class_start.astype(np.int32), fold[order].astype(np.int32), train_rows.astype(np.int32),
            (train_rows > 0).sum(axis=0).astype(np.int32))


def confidence_counts_folds(calculator: SimilarityCalculator, fold_sorted, train_rows, train_classes, thresholds, atol: float = 1.e-5):
    """[F, 4, T] count tables (tp / tn / fp / fn) of the F training parts from ONE fn_confidence_counts_folds launch over the
    calculator's rows (sorted by class); raises the reference's ValueError when a pair of some training part leaves [-1, 1]."""
    lib = _lib.load()
    thr = _ascending_f32(thresholds)
    F = int(len(train_classes))
    n, E = calculator.emb.shape
    if np.shape(train_rows) != (calculator.nrof_classes, F) or np.shape(fold_sorted) != (n,):
        raise ValueError("fold tables do not match the calculator's rows and classes")
    dev = calculator.emb.device
    as_dev = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a, dtype=dt), device=dev)
    t_dev, fold_dev = as_dev(thr, np.float32), as_dev(fold_sorted, np.int32)
    rows_dev, classes_dev = as_dev(train_rows, np.int32), as_dev(train_classes, np.int32)
    out = torch.zeros(F * 4 * thr.size, dtype=torch.float64, device=dev)
    rng = torch.zeros(2, dtype=torch.int32, device=dev)
    _lib.check(lib.fn_confidence_counts_folds(ptr(calculator.emb), ptr(calculator._cls), ptr(fold_dev), ptr(rows_dev), ptr(classes_dev),
                                              calculator.nrof_classes, E, F, ptr(t_dev), thr.size, calculator.metric, ptr(out), ptr(rng), stream(dev)),
               "confidence_counts_folds")
    counts = out.cpu().numpy().reshape(F, 4, thr.size)
    check_unit_range(rng, atol)
    return counts


class FaceToFaceValidation:
    """Interface of statistics.py:237-331: k-fold (KFold(shuffle=True, random_state=0) over image indices); per fold the
    max-accuracy and the FAR-target thresholds are chosen on the training part and scored on the held-out part.
    ``config``: .metric, .nrof_folds, .far_target.  Embeddings stay on the device.  The count tables of all training parts
    come from one fn_confidence_counts_folds launch over all rows; the held-out matrices are one
    fn_confidence_counts launch each.  Outside the kernel's range (folds > 16) every training part is a launch of its own,
    which is also what ``one_pass=False`` selects: the reference path of the tests and of tools/bench_validation.py."""

    _UPPER = {0: 4, 1: np.pi}       # largest possible similarity value per metric (statistics.py:253-258)

    def __init__(self, embeddings, labels, config, device: str = "cuda", one_pass: bool = True):
        import time
        t0 = time.monotonic()
        self.config = config
        if config.metric not in self._UPPER:
            raise ValueError('Undefined similarity metric {}'.format(config.metric))
        self.labels = np.asarray(labels)
        emb = embeddings if torch.is_tensor(embeddings) else torch.as_tensor(np.asarray(embeddings))
        self.embeddings = emb.to(device=device, dtype=torch.float32)
        assert self.embeddings.shape[0] == len(self.labels)
        self.thresholds = np.linspace(0, self._UPPER[config.metric], 100)
        self.reports = (Report(criterion='MaximumAccuracy'),
                        Report(criterion='FalseAlarmRate(FAR = {})'.format(config.far_target)))
        self.one_pass = bool(one_pass) and 2 <= config.nrof_folds <= ONE_PASS_MAX_FOLDS and len(self.thresholds) <= ONE_PASS_MAX_THRESHOLDS
        self._evaluate()
        self.elapsed_time = time.monotonic() - t0

    def _calculator(self, subset) -> SimilarityCalculator:
        dev = self.embeddings.device
        return SimilarityCalculator(self.embeddings[torch.as_tensor(subset, device=dev)], self.labels[subset],
                                    metric=self.config.metric, device=str(dev))

    def _fold_thresholds(self, matrix: ConfidenceMatrix):
        """(threshold of maximal accuracy, threshold where the false-alarm rate reaches far_target or 0)."""
        best = self.thresholds[int(np.argmax(matrix.accuracy))]
        fpr = matrix.fp_rates
        far = far_threshold_slinear(fpr, self.thresholds, self.config.far_target) if fpr.max() >= self.config.far_target else 0
        return best, far

    def _evaluate(self):
        fold, splits = kfold_assignment(len(self.labels), self.config.nrof_folds)
        if self.one_pass:
            _, _, fold_sorted, train_rows, train_classes = fold_tables(self.labels, fold, self.config.nrof_folds)
            everything = SimilarityCalculator(self.embeddings, self.labels, metric=self.config.metric, device=str(self.embeddings.device))
            tables = confidence_counts_folds(everything, fold_sorted, train_rows, train_classes, self.thresholds)
        for f, (train_set, test_set) in enumerate(splits):
            if self.one_pass:
                fitted = ConfidenceMatrix.from_counts(tables[f], self.thresholds)
            else:
                fitted = ConfidenceMatrix(self._calculator(train_set), self.thresholds)
            held_out = self._calculator(test_set)
            for report, thr in zip(self.reports, self._fold_thresholds(fitted)):
                report.append_fold('train', fitted)
                report.append_fold('test', ConfidenceMatrix(held_out, thr))

    def _text(self, header: str, footer: str = '') -> str:
        return header + 'metric: {}\n\n'.format(self.config.metric) + ''.join(str(r) for r in self.reports) + footer

    def __repr__(self):
        return self._text(f'{self.__class__.__name__}\n', f'elapsed_time: {self.elapsed_time}\n')

    @property
    def dict(self):
        return {r.criterion: r.dict for r in self.reports}

    def write_report(self, file):
        import datetime
        from pathlib import Path
        with Path(file).expanduser().open('at') as f:
            f.write(self._text(64 * '-' + '\n' + '{} {}\n'.format(self.__class__.__name__, datetime.datetime.now())))


# ------------------------------------------------------------------------------------------------------------------
# The exact verification curve: TAR at FAR, EER, ROC and AUC over ALL pairs.  A distance is the
# same bits in every pass (csrc/pair_tiles.h), so the (m + 1)-th smallest impostor distance is found by radix selection
# over recomputed distances: fn_pair_key_histogram counts the pairs of a few key windows, the host narrows a key interval
# per target and asks for finer windows.  The descent itself is a pure function of (windows) -> counts.
# ------------------------------------------------------------------------------------------------------------------
KEY_BINS = 1024                  # bins per window of fn_pair_key_histogram
KEY_WINDOWS = 8                  # windows per launch
KEY_TOP = {0: 0x40800000, 1: 0x40490FDB}       # the key of the largest distance: 4.0 and fp32 pi (FaceToFaceValidation._UPPER)
# The first pass: the octaves [2, 4), [1, 2), ... [2^-6, 2^-5), 1024 bins of 2^13 keys each.  One window that is linear in the key
# over [0, 4] has bins half a unit wide at d = 2: a useless ROC and a descent of four passes (shift 21, 11, 1, 0); from an octave
# bin it takes three (13, 3, 0).  What lies below 2^-6 is one "below" count, and a target there takes four passes.
FIRST_WINDOWS = ([0x40000000 - (j << 23) for j in range(KEY_WINDOWS)], [13] * KEY_WINDOWS)


def f32_key(x) -> int:
    """The bit pattern of an fp32 value >= +0 as an integer: keys order as the values do."""
    return int(np.array([x], dtype=np.float32).view(np.uint32)[0])


def key_f32(key: int) -> float:
    return float(np.array([key], dtype=np.uint32).view(np.float32)[0])


class KeyTarget:
    """One key the descent looks for: the largest key k with ``low(cumG(k), cumI(k))``, cumG / cumI the numbers of genuine /
    impostor pairs whose key is below k.  ``low`` is true at key 0, false above the largest key and never true after it was
    false.  The key lies in [klo, khi]; at_lo / at_hi are (cumG, cumI) at klo and at khi + 1."""

    __slots__ = ("low", "klo", "khi", "at_lo", "at_hi")

    def __init__(self, low, top: int, totals):
        self.low, self.klo, self.khi, self.at_lo, self.at_hi = low, 0, int(top), (0, 0), tuple(int(v) for v in totals)

    @property
    def found(self):
        return self.klo == self.khi


def window_counts(counts):
    """uint64 [2, KEY_BINS + 2] of one window -> uint64 [2, KEY_BINS + 1]: the pairs below each of the window's bin edges."""
    counts = np.asarray(counts, dtype=np.uint64)
    cum = np.empty((2, KEY_BINS + 1), dtype=np.uint64)
    cum[:, 0] = counts[:, KEY_BINS]
    cum[:, 1:] = counts[:, KEY_BINS, None] + np.cumsum(counts[:, :KEY_BINS], axis=1, dtype=np.uint64)
    return cum


def narrow(target: KeyTarget, lo: int, shift: int, cum):
    """Intersect the target's interval with what one window's edge counts say (edge b is the key lo + (b << shift))."""
    at = lambda b: (int(cum[0, b]), int(cum[1, b]))
    if not target.low(*at(0)):
        b = -1                                           # the key is below the window
    else:
        b, top = 0, KEY_BINS                             # the last edge that is still low
        while b < top:
            mid = (b + top + 1) // 2
            if target.low(*at(mid)):
                b = mid
            else:
                top = mid - 1
    if b >= 0 and lo + (b << shift) > target.klo:
        target.klo, target.at_lo = lo + (b << shift), at(b)
    if b < KEY_BINS and lo + ((b + 1) << shift) - 1 < target.khi:
        target.khi, target.at_hi = lo + ((b + 1) << shift) - 1, at(b + 1)
    if target.klo > target.khi:
        raise RuntimeError("key descent: the counts of two passes contradict each other")


def key_descent(histogram, targets, first=None) -> int:
    """Find every target.  ``histogram(lo, shift)`` -> uint64 [R, 2, KEY_BINS + 2] as fn_pair_key_histogram fills it, for R <= 8
    windows.  Targets are refined together in groups of 8, one window each: the window starts at klo and takes the smallest
    shift that covers [klo, khi], so an interval of n keys shrinks to n / 1024 per pass.  Every window of a pass informs every
    open target.  ``first``: (lo, shift, counts) of a pass that has been run already.  -> the number of passes run."""
    def apply(lo, shift, counts):
        for r in range(len(lo)):
            cum = window_counts(counts[r])
            for t in targets:
                if not t.found:
                    narrow(t, int(lo[r]), int(shift[r]), cum)

    if first is not None:
        apply(*first)
    passes = 0
    for g in range(0, len(targets), KEY_WINDOWS):
        group = targets[g:g + KEY_WINDOWS]
        while True:
            todo = [t for t in group if not t.found]
            if not todo:
                break
            lo = [t.klo for t in todo]
            shift = [max(0, (t.khi - t.klo).bit_length() - 10) for t in todo]        # the smallest with (khi - klo) >> shift < 1024
            apply(lo, shift, np.asarray(histogram(lo, shift)))
            passes += 1
    return passes


class VerificationCurve:
    """The exact verification curve of a set of embeddings: every unordered pair of distinct rows is evaluated once, genuine when
    both rows carry one label and impostor otherwise; d is the distance ``Gallery`` and ``ConfidenceMatrix`` compute, bit for
    bit (``pairwise_similarities`` sums in another order: equal to rounding only), and a pair is accepted at threshold t when
    d < t (strict fp32), as every consumer decides.  ``tar_at_far`` gives the largest threshold whose false accepts stay within f
    times the impostor pairs; integers are exact, ratios are formed from them."""

    def __init__(self, embeddings, labels, metric=0, device: str = "cuda", atol: float = 1.e-5):
        if metric not in KEY_TOP:
            raise ValueError('Undefined similarity metric {}'.format(metric))
        sizes = [int(c) for c in np.unique(np.asarray(labels), return_counts=True)[1]]
        n = sum(sizes)
        genuine = sum(c * (c - 1) // 2 for c in sizes)
        self._init(self._device_histogram, genuine, n * (n - 1) // 2 - genuine, metric)      # rejects an empty population: no launch
        calc = SimilarityCalculator(embeddings, labels, metric=metric, device=device)
        emb = calc.emb
        if emb.shape[1] % 4:       # zeros add fma(0, 0, acc) = acc: no bit of a dot product changes
            emb = torch.nn.functional.pad(emb, (0, 4 - emb.shape[1] % 4)).contiguous()
        self._emb, self._cls, self._classes, self._atol = emb, calc._cls, calc.nrof_classes, atol

    @classmethod
    def from_histogram(cls, histogram, nrof_genuine: int, nrof_impostor: int, metric=0):
        """A curve over any ``histogram(lo, shift)`` that counts like fn_pair_key_histogram (the tests' NumPy stand-in)."""
        self = cls.__new__(cls)
        self._init(histogram, nrof_genuine, nrof_impostor, metric)
        return self

    def _init(self, histogram, nrof_genuine, nrof_impostor, metric):
        if metric not in KEY_TOP:
            raise ValueError('Undefined similarity metric {}'.format(metric))
        self.metric, self.nrof_genuine, self.nrof_impostor = metric, int(nrof_genuine), int(nrof_impostor)
        if self.nrof_genuine < 1 or self.nrof_impostor < 1:
            raise ValueError("a verification curve needs genuine and impostor pairs, got {} and {}".format(self.nrof_genuine,
                                                                                                            self.nrof_impostor))
        self._histogram = histogram
        self.nrof_passes = 0          # launches so far
        self.nrof_groups = 0          # groups of <= 8 targets refined so far
        self._first = None            # (lo, shift, counts) of the first pass
        self._far, self._eer, self._asked, self._buffer = {}, None, {}, None

    def _device_histogram(self, lo, shift):
        """One launch.  `out` and the two `range` words share one buffer, allocated once per curve: a pass costs one fill and one
        transfer to the host, its only synchronisation."""
        import ctypes
        lib = _lib.load()
        R, words = len(lo), len(lo) * 2 * (KEY_BINS + 2)
        dev = self._emb.device
        if self._buffer is None:
            self._buffer = torch.empty(KEY_WINDOWS * 2 * (KEY_BINS + 2) + 1, dtype=torch.int64, device=dev)
        buf = self._buffer[:words + 1]
        buf.zero_()
        _lib.check(lib.fn_pair_key_histogram(ptr(self._emb), ptr(self._cls), self._classes, self._emb.shape[1], self.metric,
                                             (ctypes.c_uint32 * R)(*lo), (ctypes.c_int32 * R)(*shift), R, ptr(buf), ptr(buf, words), stream(dev)),
                   "pair_key_histogram")
        host = buf.cpu()
        check_unit_range(host[words:].view(torch.int32), self._atol)
        return host[:words].numpy().view(np.uint64).reshape(R, 2, KEY_BINS + 2)

    # ---- the passes --------------------------------------------------------------------------------------------------------
    def _first_pass(self):
        if self._first is None:
            lo, shift = FIRST_WINDOWS
            counts = np.asarray(self._histogram(lo, shift))
            self.nrof_passes += 1
            if [int(v) for v in counts[0, :, KEY_BINS + 1]] != [self.nrof_genuine, self.nrof_impostor]:
                raise RuntimeError("pair_key_histogram counted {} pairs, the labels give {}".format(
                    counts[0, :, KEY_BINS + 1].tolist(), [self.nrof_genuine, self.nrof_impostor]))
            self._first = (lo, shift, counts)
        return self._first

    def _target(self, low):
        return KeyTarget(low, KEY_TOP[self.metric], (self.nrof_genuine, self.nrof_impostor))

    def _resolve(self, ranks=()):
        """Find the thresholds of the impostor ranks that are not known yet, and the EER with them."""
        new = []
        if self._eer is None:
            Gn, I = self.nrof_genuine, self.nrof_impostor
            self._eer = self._target(lambda g, i: i * Gn < (Gn - g) * I)
            new.append(self._eer)
        for m in ranks:
            if m not in self._far:
                self._far[m] = self._target(lambda g, i, m=m: i <= m)
                new.append(self._far[m])
        if new:
            first = self._first_pass()
            self.nrof_passes += key_descent(self._histogram, new, first=first)
            self.nrof_groups += -(-len(new) // KEY_WINDOWS)

    # ---- the public interface ----------------------------------------------------------------------------------------------
    def tar_at_far(self, fars):
        """One record per false-accept rate f, ascending in [0, 1]: m = int(f * impostor pairs) in exact arithmetic, ``threshold``
        the (m + 1)-th smallest impostor distance (the largest fp32 t with at most m impostor pairs d < t; +inf when m reaches
        the number of impostor pairs), ``false_accepts`` / ``true_accepts`` the impostor / genuine pairs with d < threshold (ties
        may leave false_accepts below m), ``far`` and ``tar`` their shares."""
        from fractions import Fraction
        fars = [float(f) for f in np.atleast_1d(np.asarray(fars, dtype=np.float64))]
        if any(not 0.0 <= f <= 1.0 for f in fars):
            raise ValueError("false-accept rates must lie in [0, 1], got {}".format(fars))
        if any(b < a for a, b in zip(fars, fars[1:])):
            raise ValueError("false-accept rates must be ascending, got {}".format(fars))
        Gn, I = self.nrof_genuine, self.nrof_impostor
        ranks = [int(Fraction(f) * I) for f in fars]
        self._resolve([m for m in ranks if m < I])
        records = []
        for f, m in zip(fars, ranks):
            if m < I:
                t, (ta, fa) = key_f32(self._far[m].klo), self._far[m].at_lo
            else:
                t, ta, fa = float("inf"), Gn, I
            self._asked[f] = {"far_target": f, "threshold": t, "false_accepts": fa, "true_accepts": ta, "far": fa / I, "tar": ta / Gn}
            records.append(dict(self._asked[f]))
        return records

    def threshold_at_far(self, f) -> float:
        return self.tar_at_far([f])[0]["threshold"]

    def eer(self):
        """``eer_threshold``: the smallest fp32 t whose false-accept share reaches its false-reject share (compared in
        integers); ``far`` and ``frr`` there, ``eer`` their mean."""
        self._resolve()
        Gn, I = self.nrof_genuine, self.nrof_impostor
        ta, fa = self._eer.at_hi                              # one key above the last one that is still low
        far, frr = fa / I, (Gn - ta) / Gn
        return {"eer": (far + frr) / 2, "eer_threshold": key_f32(self._eer.klo + 1), "far": far, "frr": frr, "false_accepts": fa,
                "true_accepts": ta}

    def roc_counts(self):
        """(keys, true_accepts, false_accepts), Python integers: the pairs with a key below each bin edge of the first pass, key 0
        and the key above the largest distance included."""
        lo, shift, counts = self._first_pass()
        at = {0: (0, 0), KEY_TOP[self.metric] + 1: (self.nrof_genuine, self.nrof_impostor)}
        for r in range(len(lo)):
            cum = window_counts(counts[r])
            for b in range(KEY_BINS + 1):
                key = lo[r] + (b << shift[r])
                if key <= KEY_TOP[self.metric]:
                    at[key] = (int(cum[0, b]), int(cum[1, b]))
        keys = sorted(at)
        return keys, [at[k][0] for k in keys], [at[k][1] for k in keys]

    def roc(self):
        """(far, tar, threshold), ascending: the exact shares of impostor / genuine pairs with d < threshold at every bin edge of
        the first pass (float64, float64, float32 arrays)."""
        keys, ta, fa = self.roc_counts()
        return (np.array([v / self.nrof_impostor for v in fa]), np.array([v / self.nrof_genuine for v in ta]),
                np.array(keys, dtype=np.uint32).view(np.float32))

    def auc(self):
        """(auc, auc_lo, auc_hi): the share of (genuine, impostor) pairs of pairs the genuine one of which is nearer, ties counted
        1/2, lies in [auc_lo, auc_hi]: pairs of pairs that share a bin of the first pass are left out of auc_lo and counted in
        auc_hi; auc is the midpoint.  Exact integers up to the last division."""
        from fractions import Fraction
        _, ta, fa = self.roc_counts()
        Gn, I = self.nrof_genuine, self.nrof_impostor
        above = sum((ta[b + 1] - ta[b]) * (I - fa[b + 1]) for b in range(len(ta) - 1))
        tied = sum((ta[b + 1] - ta[b]) * (fa[b + 1] - fa[b]) for b in range(len(ta) - 1))
        lo, hi = Fraction(above, Gn * I), Fraction(above + tied, Gn * I)
        return float((lo + hi) / 2), float(lo), float(hi)

    def dict(self):
        auc, auc_lo, auc_hi = self.auc()
        out = {"metric": self.metric, "nrof_genuine": self.nrof_genuine, "nrof_impostor": self.nrof_impostor, "auc": auc,
               "auc_lo": auc_lo, "auc_hi": auc_hi}
        out.update(self.eer())
        out["tar_at_far"] = [dict(self._asked[f]) for f in sorted(self._asked)]
        return out

    def __repr__(self):
        d = self.dict()
        text = ('{}\nmetric: {}\n\ngenuine pairs: {}\nimpostor pairs: {}\nArea under curve (AUC): {:1.5f} [{:1.5f}, {:1.5f}]\n'
                'Equal error rate (EER): {:1.5f}\nThreshold: {:2.5f}\n\n').format(
                    self.__class__.__name__, d["metric"], d["nrof_genuine"], d["nrof_impostor"], d["auc"], d["auc_lo"], d["auc_hi"],
                    d["eer"], d["eer_threshold"])
        for r in d["tar_at_far"]:
            text += ('TAR @ FAR = {}\nTrue accept rate (TAR):  {:1.5f} ({} of {})\nFalse accept rate (FAR): {:.3e} ({} of {})\n'
                     'Threshold: {:2.5f}\n\n').format(r["far_target"], r["tar"], r["true_accepts"], d["nrof_genuine"], r["far"],
                                                      r["false_accepts"], d["nrof_impostor"], r["threshold"])
        return text


def verification_curve(embeddings, labels, config, device: str = "cuda"):
    """The curve ``config.far_targets`` asks for (a list of false-accept rates, ascending), evaluated; None when the key is unset:
    the one helper of apps/validate.py and ValidateCallback."""
    from .config import Config
    fars = getattr(config, "far_targets", None)
    if fars is None or isinstance(fars, Config):        # a Config reads a missing key as an empty Config
        return None
    curve = VerificationCurve(embeddings, labels, metric=config.metric, device=device)
    curve.tar_at_far(sorted(float(f) for f in np.atleast_1d(fars)))
    curve.eer()
    return curve


# ------------------------------------------------------------------------------------------------------------------
# Open-set 1:N identification: FNIR at FPIR, the detection-and-identification rate and the CMC at any
# rank, from each probe's nearest mate, nearest impostor and rank (Gallery.mates / fn_mate_search).  The 1:N sibling of
# VerificationCurve: integers are exact, ratios are formed from them.
# ------------------------------------------------------------------------------------------------------------------
class IdentificationCurve:
    """The leave-one-out open-set identification curve of a set of embeddings (ISO/IEC 19795-1, the FNIR at FPIR of 1:N
    evaluations).  Every row is a probe against all other rows.  MATED searches: the probes whose class has another image
    (``nrof_mated`` = M); such a probe is a hit at (threshold t, rank R) when fewer than R impostor rows are nearer than its
    nearest mate and that mate's distance d < t (strict fp32, as `Gallery.identify` decides).  NON-MATED searches: the same
    probe against the gallery without its whole identity, whose top candidate is exactly the nearest impostor
    (``nrof_nonmated`` = N probes that have one: all of them with two or more classes); it is a false positive when that
    distance d < t.  Distances are `Gallery.search`'s bit for bit."""

    def __init__(self, embeddings, labels, metric=0, device: str = "cuda", atol: float = 1.e-5):
        if metric not in KEY_TOP:
            raise ValueError('Undefined similarity metric {}'.format(metric))
        labels = host_array(labels)
        _, inverse, sizes = np.unique(labels, return_inverse=True, return_counts=True)
        n = len(labels)
        self._check(int(np.count_nonzero(sizes[inverse.reshape(-1)] > 1)) if n else 0, n if len(sizes) > 1 else 0)      # no launch
        gallery = Gallery(embeddings, labels=inverse.reshape(-1).astype(np.int64), metric=metric, device=device)
        found = gallery.mates(gallery.embeddings, gallery.labels, skip=np.arange(n, dtype=np.int32), ranks=True, atol=atol)
        self._init(*(t.cpu().numpy() for t in found), metric)

    @classmethod
    def from_search(cls, mate_dist, impostor_dist, ranks, metric=0, impostor_rows=None):
        """The curve over host arrays, one entry per probe: what `Gallery.mates` returned for a real probe set, or the tests'
        NumPy stand-in.  A probe is mated when ranks >= 0 and non-mated scored when its impostor distance is finite."""
        self = cls.__new__(cls)
        if metric not in KEY_TOP:
            raise ValueError('Undefined similarity metric {}'.format(metric))
        mate_dist, impostor_dist, ranks = np.asarray(mate_dist), np.asarray(impostor_dist), np.asarray(ranks)
        if not (mate_dist.ndim == 1 and mate_dist.shape == impostor_dist.shape == ranks.shape) or ranks.dtype.kind not in "iu":
            raise ValueError("from_search: mate_dist, impostor_dist and integer ranks must be 1-D and of equal length, got {}, {} and {} of {}"
                             .format(mate_dist.shape, impostor_dist.shape, ranks.shape, ranks.dtype))
        if impostor_rows is None:
            impostor_rows = np.full(ranks.shape, -1, np.int32)
        self._check(int(np.count_nonzero(ranks >= 0)), int(np.count_nonzero(np.isfinite(impostor_dist.astype(np.float32)))))
        self._init(mate_dist, np.full(ranks.shape, -1, np.int32), impostor_dist, impostor_rows, ranks, metric)
        return self

    @staticmethod
    def _check(mated, nonmated):
        if mated < 1 or nonmated < 1:
            raise ValueError("an identification curve needs mated and non-mated searches, got {} and {}".format(mated, nonmated))

    def _init(self, mate_dist, mate_rows, impostor_dist, impostor_rows, ranks, metric):
        self.metric = metric
        self.mate_dist, self.impostor_dist = np.asarray(mate_dist, dtype=np.float32), np.asarray(impostor_dist, dtype=np.float32)
        self.mate_rows, self.impostor_rows = np.asarray(mate_rows), np.asarray(impostor_rows)
        self.ranks = np.asarray(ranks).astype(np.int64)
        self.nrof_probes = len(self.ranks)
        self.nrof_mated = int(np.count_nonzero(self.ranks >= 0))
        self._sorted = np.sort(self.impostor_dist[np.isfinite(self.impostor_dist)])          # the non-mated scores, ascending
        self.nrof_nonmated = len(self._sorted)
        self._asked = {}

    def _counts(self, threshold, rank):
        t = np.float32(threshold)
        false_positives = int(np.searchsorted(self._sorted, t, side="left"))                  # #{d < t}
        hits = int(np.count_nonzero((self.ranks >= 0) & (self.ranks < rank) & (self.mate_dist < t)))
        M, N = self.nrof_mated, self.nrof_nonmated
        return {"threshold": float(t), "rank": rank, "false_positives": false_positives, "hits": hits, "fpir": false_positives / N,
                "dir": hits / M, "fnir": 1 - hits / M}

    def fnir_at_fpir(self, fpirs, rank=1):
        """One record per false-positive identification rate f, ascending in [0, 1]: m = int(f * N) in exact arithmetic,
        ``threshold`` the (m + 1)-th smallest nearest-impostor distance (the largest fp32 t with at most m false positives; +inf
        when m reaches N), ``false_positives`` the non-mated searches with d < threshold (ties may leave it below m), ``hits``
        the mated searches with the mate within ``rank`` and nearer than the threshold; ``fpir``, ``dir`` (the detection and
        identification rate) and ``fnir`` = 1 - dir their shares."""
        from fractions import Fraction
        rank = check_int("rank", rank, 1)
        fpirs = [float(f) for f in np.atleast_1d(np.asarray(fpirs, dtype=np.float64))]
        if any(not 0.0 <= f <= 1.0 for f in fpirs):
            raise ValueError("false-positive identification rates must lie in [0, 1], got {}".format(fpirs))
        if any(b < a for a, b in zip(fpirs, fpirs[1:])):
            raise ValueError("false-positive identification rates must be ascending, got {}".format(fpirs))
        records = []
        for f in fpirs:
            m = int(Fraction(f) * self.nrof_nonmated)
            t = self._sorted[m] if m < self.nrof_nonmated else np.float32(np.inf)
            record = {"fpir_target": f}
            record.update(self._counts(t, rank))
            self._asked[(f, rank)] = record
            records.append(dict(record))
        return records

    def dir_at(self, threshold, rank=1):
        """The counts of `fnir_at_fpir` at a threshold of the caller's: a classifier's, or `VerificationCurve.threshold_at_far`."""
        rank = check_int("rank", rank, 1)
        if np.isnan(np.float32(threshold)):
            raise ValueError("threshold must be a number, got NaN")
        return self._counts(threshold, rank)

    def cmc(self, k):
        """-> (curve float64 [k], left_out): curve[r] is the share of mated probes whose first mate has rank <= r, at any depth;
        for k <= 64 it is `statistics.cmc` of the leave-one-out search."""
        k = check_int("k", k, 1)
        mated = self.ranks[self.ranks >= 0]
        found = np.cumsum(np.bincount(np.minimum(mated, k), minlength=k + 1)[:k])
        return found / np.float64(self.nrof_mated), self.nrof_probes - self.nrof_mated

    def mislabelled(self):
        """The probes whose nearest impostor precedes their nearest mate, as (row, impostor row, mate distance, impostor
        distance), nearest impostor first: the label-noise shortlist of a data set."""
        bad = np.nonzero(self.ranks > 0)[0]
        bad = bad[np.lexsort((bad, self.impostor_dist[bad]))]
        return [(int(i), int(self.impostor_rows[i]), float(self.mate_dist[i]), float(self.impostor_dist[i])) for i in bad]

    def dict(self):
        curve, left_out = self.cmc(1)
        return {"metric": self.metric, "nrof_probes": self.nrof_probes, "nrof_mated": self.nrof_mated, "nrof_nonmated": self.nrof_nonmated,
                "left_out": left_out, "rank1": float(curve[0]), "nrof_mislabelled": int(np.count_nonzero(self.ranks > 0)),
                "fnir_at_fpir": [dict(self._asked[key]) for key in sorted(self._asked)]}

    def __repr__(self):
        d = self.dict()
        text = ('{}\nmetric: {}\n\nmated searches: {}\nnon-mated searches: {}\nRank-1 identification rate (closed set): {:1.5f}\n'
                'Probes nearer to an impostor than to a mate: {}\n\n').format(self.__class__.__name__, d["metric"], d["nrof_mated"],
                                                                             d["nrof_nonmated"], d["rank1"], d["nrof_mislabelled"])
        for r in d["fnir_at_fpir"]:
            text += ('FNIR @ FPIR = {} (rank {})\nFalse negative identification rate (FNIR): {:1.5f} ({} of {} missed)\n'
                     'False positive identification rate (FPIR): {:.3e} ({} of {})\nThreshold: {:2.5f}\n\n').format(
                         r["fpir_target"], r["rank"], r["fnir"], d["nrof_mated"] - r["hits"], d["nrof_mated"], r["fpir"],
                         r["false_positives"], d["nrof_nonmated"], r["threshold"])
        return text


def identification_curve(embeddings, labels, config, device: str = "cuda"):
    """The curve ``config.fpir_targets`` asks for (a list of false-positive identification rates; ``config.fpir_rank``, default 1),
    evaluated; None when the key is unset: the one helper of apps/validate.py and ValidateCallback."""
    from .config import Config
    fpirs = getattr(config, "fpir_targets", None)
    if fpirs is None or isinstance(fpirs, Config):        # a Config reads a missing key as an empty Config
        return None
    rank = getattr(config, "fpir_rank", None)
    rank = 1 if rank is None or isinstance(rank, Config) else check_int("rank", rank, 1)
    fpirs = sorted(float(f) for f in np.atleast_1d(fpirs))
    if any(not 0.0 <= f <= 1.0 for f in fpirs):           # before any launch
        raise ValueError("false-positive identification rates must lie in [0, 1], got {}".format(fpirs))
    curve = IdentificationCurve(embeddings, labels, metric=config.metric, device=device)
    curve.fnir_at_fpir(fpirs, rank=rank)
    return curve


# Which pairs a threshold gets wrong: a module of its own, on SimilarityCalculator
from .false_examples import FalseExamples, false_examples      # noqa: E402, F401
