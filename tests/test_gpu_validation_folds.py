"""fn_confidence_counts_folds (the count tables of all training parts of a k-fold validation in one pass, DESIGN.md section
16) against fn_confidence_counts run per fold, against the CPU restatement of the reference, and FaceToFaceValidation on
the one-pass path against the per-fold path and the reference."""
import numpy as np
import pytest
import torch

from facenet_amd.config import Config
from facenet_amd.statistics import (ConfidenceMatrix, FaceToFaceValidation, SimilarityCalculator, confidence_counts_folds, fold_tables,
                                    kfold_assignment)
from oracle import statistics_oracle as so
from tests import validation_folds_oracle as vo

pytestmark = pytest.mark.gpu

ROWS = ("tp", "tn", "fp", "fn")


def _one_pass(emb, labels, F, metric, thr):
    fold, splits = kfold_assignment(len(labels), F)
    _, _, fold_sorted, train_rows, train_classes = fold_tables(labels, fold, F)
    tables = confidence_counts_folds(SimilarityCalculator(emb, labels, metric), fold_sorted, train_rows, train_classes, thr)
    return tables, splits, train_rows


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("sizes,E,F,vanished", vo.CASES)
def test_tables_equal_the_per_fold_kernel(sizes, E, F, vanished, metric):
    """Both kernels bin identical distances, so the integer counts agree and the tables differ only by the order of at most
    C(C+1)/2 non-negative fp64 additions per entry."""
    emb, labels = vo.pool(sizes, E, seed=len(sizes))
    thr = np.linspace(0, 4 if metric == 0 else np.pi, 100)
    tables, splits, train_rows = _one_pass(emb, labels, F, metric, thr)
    assert tables.shape == (F, 4, 100) and int((train_rows == 0).sum()) == vanished
    C = len(sizes)
    rel = C * (C + 1) / 2 * 2.0 ** -52
    for f, (train, _) in enumerate(splits):
        ref = ConfidenceMatrix(SimilarityCalculator(emb[train], labels[train], metric), thr)
        diff = np.abs(tables[f] - ref.counts)
        print(sizes[:4], E, F, metric, "fold", f, "max rel diff", float((diff / np.maximum(np.abs(ref.counts), 1e-300)).max()), "bound", rel)
        assert np.all(diff <= rel * np.abs(ref.counts)), (f, float(diff.max()))


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("sizes,E,F,vanished", vo.CASES)
def test_tables_match_the_reference_loops(sizes, E, F, vanished, metric):
    emb, labels = vo.pool(sizes, E, seed=len(sizes))
    thr = np.linspace(0, 4 if metric == 0 else np.pi, 100)
    tables, splits, _ = _one_pass(emb, labels, F, metric, thr)
    for f, (train, _) in enumerate(splits):
        ref = so.ConfidenceMatrix(so.SimilarityCalculator(emb[train], labels[train], metric), thr)
        got = ConfidenceMatrix.from_counts(tables[f], thr)
        left = np.unique(labels[train], return_counts=True)[1]
        # the slack of test_confidence_matrix_matches_reference_loops for the classes and rows of this training part
        slack = 3.0 / max(1, min([n * (n - 1) // 2 for n in left if n > 1] or [1])) / len(left)
        for name in ROWS:
            assert np.allclose(getattr(got, name), getattr(ref, name), atol=max(slack, 1e-9)), (f, name)
        for name in ("accuracy", "precision", "tp_rates", "tn_rates", "fp_rates"):
            assert np.allclose(getattr(got, name), getattr(ref, name), atol=5e-3), (f, name)


def test_largest_supported_folds_and_thresholds():
    """F = 16 and T = 256 are the kernel's limits (its largest LDS footprint); one past either is refused."""
    emb, labels = vo.pool([9, 20, 5, 70, 3], 40, seed=9)
    thr = np.linspace(0, 4, 256)
    tables, splits, _ = _one_pass(emb, labels, 16, 0, thr)
    for f, (train, _) in enumerate(splits):
        ref = ConfidenceMatrix(SimilarityCalculator(emb[train], labels[train], 0), thr)
        assert np.all(np.abs(tables[f] - ref.counts) <= 15 * 2.0 ** -52 * np.abs(ref.counts)), f
    fold, _ = kfold_assignment(len(labels), 17)
    _, _, fs, rows, classes = fold_tables(labels, fold, 17)
    with pytest.raises(ValueError):
        confidence_counts_folds(SimilarityCalculator(emb, labels, 0), fs, rows, classes, thr)
    fold, _ = kfold_assignment(len(labels), 4)
    _, _, fs, rows, classes = fold_tables(labels, fold, 4)
    with pytest.raises(ValueError):
        confidence_counts_folds(SimilarityCalculator(emb, labels, 0), fs, rows, classes, np.linspace(0, 4, 257))


def test_face_to_face_validation_on_the_one_pass_path():
    emb, labels = vo.pool([6] * 12 + [9, 3, 14], 64, seed=5)
    cfg = Config({"metric": 0, "nrof_folds": 4, "far_target": 1e-3})
    got = FaceToFaceValidation(emb, labels, cfg)
    per_fold = FaceToFaceValidation(emb, labels, cfg, one_pass=False)
    assert got.one_pass and not per_fold.one_pass
    ref = so.face_to_face_validation(emb, labels, 0, nrof_folds=4, far_target=1e-3)
    for crit, d in ref.items():
        for key, val in d.items():
            assert abs(got.dict[crit][key] - val) < 6e-3, (crit, key, got.dict[crit][key], val)
        for key in ("auc", "eer"):                         # continuous in the training tables
            assert abs(got.dict[crit][key] - per_fold.dict[crit][key]) <= 1e-9, (crit, key)
    for report in got.reports:
        assert all(isinstance(m, ConfidenceMatrix) for m in report.conf_matrix_train + report.conf_matrix_test)
        assert len(report.conf_matrix_train) == 4 and report.conf_matrix_train[0].counts.shape == (4, 100)
    text = repr(got)
    assert "MaximumAccuracy" in text and "Area under curve (AUC)" in text and "elapsed_time" in text


@pytest.mark.parametrize("one_pass", [True, False])
def test_unnormalised_embeddings_raise(one_pass):
    emb, labels = vo.pool([4, 4, 4], 64, seed=1)
    with pytest.raises(ValueError, match="embeddings must be normalized to 1"):
        FaceToFaceValidation(emb * 2.0, labels, Config({"metric": 0, "nrof_folds": 3, "far_target": 1e-3}), one_pass=one_pass)


def test_twenty_folds_take_the_per_fold_path():
    emb, labels = vo.pool([6] * 12 + [9, 3, 14], 64, seed=5)
    cfg = Config({"metric": 0, "nrof_folds": 20, "far_target": 1e-3})
    got = FaceToFaceValidation(emb, labels, cfg)
    assert not got.one_pass
    ref = FaceToFaceValidation(emb, labels, cfg, one_pass=False)
    for crit in ref.dict:                                  # the same path twice: only the order of the fp64 atomics differs
        for key in ("auc", "eer"):
            assert abs(got.dict[crit][key] - ref.dict[crit][key]) <= 1e-9, (crit, key)
