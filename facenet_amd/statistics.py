"""``pairwise_similarities`` with the reference's signature and error behaviour (facenet/statistics.py:22-57),
computed by the wavefront-reduced fn_pairwise_sqdist kernel."""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from .engine import _ptr


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
    st = torch.cuda.current_stream(a.device).cuda_stream
    _lib.check(lib.fn_pairwise_sqdist(_ptr(a), _ptr(b), _ptr(out), _ptr(rng), n, m, E, metric, st), "pairwise_sqdist")
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


class ConfidenceMatrix:
    """Interface of statistics.py:111-175 (attributes tp / tn / fp / fn / threshold, the six rate properties).  The
    class-balanced counts for ALL thresholds come from one fn_confidence_counts launch into ``counts`` [4, T]; every rate is
    a ratio of two rows of it."""

    _ROWS = {"tp": 0, "tn": 1, "fp": 2, "fn": 3}

    def __init__(self, calculator: SimilarityCalculator, threshold, atol: float = 1.e-5):
        lib = _lib.load()
        self.threshold = np.array(threshold, ndmin=1)
        thr = self.threshold.astype(np.float32)
        if thr.size > 1 and not np.all(np.diff(thr) >= 0):
            raise ValueError("thresholds must be ascending")
        dev = calculator.emb.device
        t_dev = torch.as_tensor(thr, device=dev)
        out = torch.zeros(4 * thr.size, dtype=torch.float64, device=dev)
        rng = torch.zeros(2, dtype=torch.int32, device=dev)
        n, E = calculator.emb.shape
        st = torch.cuda.current_stream(dev).cuda_stream
        _lib.check(lib.fn_confidence_counts(_ptr(calculator.emb), _ptr(calculator._cls), calculator.nrof_classes, E, _ptr(t_dev), thr.size,
                                            calculator.metric, _ptr(out), _ptr(rng), st), "confidence_counts")
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
    thr = np.array(thresholds, ndmin=1).astype(np.float32)
    if thr.size > 1 and not np.all(np.diff(thr) >= 0):
        raise ValueError("thresholds must be ascending")
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
    st = torch.cuda.current_stream(dev).cuda_stream
    _lib.check(lib.fn_confidence_counts_folds(_ptr(calculator.emb), _ptr(calculator._cls), _ptr(fold_dev), _ptr(rows_dev), _ptr(classes_dev),
                                              calculator.nrof_classes, E, F, _ptr(t_dev), thr.size, calculator.metric, _ptr(out), _ptr(rng), st),
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
