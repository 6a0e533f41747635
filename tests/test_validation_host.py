"""Host side of the one-pass k-fold validation and of validation inside training: the NumPy
restatement of the one-pass arithmetic against the reference loops per fold, the host tables of the kernel, the epoch rule and
the bookkeeping of ValidateCallback, the config defaults, the validate app's options and the rank sharding."""
import numpy as np
import pytest

from facenet_amd import callbacks
from facenet_amd.config import Config, load_config
from facenet_amd.statistics import ConfidenceMatrix, fold_tables, kfold_assignment
from oracle import statistics_oracle as so
from tests import validation_folds_oracle as vo


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("sizes,E,F,vanished", vo.CASES)
def test_one_pass_arithmetic_equals_the_reference_per_fold(sizes, E, F, vanished, metric):
    emb, labels = vo.pool(sizes, E, seed=len(sizes))
    thr = np.linspace(0, 4 if metric == 0 else np.pi, 100)
    fold, splits = vo.kfold(len(labels), F)
    got, cells = vo.onepass(emb, labels, fold, thr, F, metric)
    assert cells == vanished                          # the vanishing-class sets must stay what they are
    for f, (train, _) in enumerate(splits):
        ref = so.ConfidenceMatrix(so.SimilarityCalculator(emb[train].astype(np.float64), labels[train], metric), thr)
        for r, name in enumerate(("tp", "tn", "fp", "fn")):
            assert np.abs(got[f, r] - getattr(ref, name)).max() <= 1e-12, (f, name)


@pytest.mark.parametrize("sizes,E,F,vanished", vo.CASES)
def test_host_tables_against_brute_force(sizes, E, F, vanished):
    _, labels = vo.pool(sizes, E, seed=len(sizes))
    fold, splits = kfold_assignment(len(labels), F)
    want_fold, want_splits = vo.kfold(len(labels), F)
    assert np.array_equal(fold, want_fold) and fold.dtype == np.int32
    for (a, b), (c, d) in zip(splits, want_splits):
        assert np.array_equal(a, c) and np.array_equal(b, d)
    order, class_start, fold_sorted, train_rows, train_classes = fold_tables(labels, fold, F)
    assert np.array_equal(labels[order], np.sort(labels)) and np.array_equal(fold_sorted, fold[order])
    assert np.array_equal(order, np.argsort(labels, kind="stable"))
    assert np.array_equal(np.diff(class_start), np.unique(labels, return_counts=True)[1]) and class_start[0] == 0
    rows, classes = vo.tables(labels, fold, F)
    assert np.array_equal(train_rows, rows) and np.array_equal(train_classes, classes)
    assert int((train_rows == 0).sum()) == vanished
    for t in (class_start, fold_sorted, train_rows, train_classes):
        assert t.dtype == np.int32
    with pytest.raises(ValueError):
        fold_tables(labels, fold + 1, F)


def test_confidence_matrix_from_counts():
    counts = np.array([[1.0, 2.0], [3.0, 1.0], [0.5, 0.0], [0.0, 2.0]])
    m = ConfidenceMatrix.from_counts(counts, [0.5, 1.0])
    assert isinstance(m, ConfidenceMatrix) and m.threshold.shape == (2,)
    assert np.array_equal(m.tp, counts[0]) and np.array_equal(m.tn, counts[1]) and np.array_equal(m.fp, counts[2]) and np.array_equal(m.fn, counts[3])
    assert np.allclose(m.accuracy, [4 / 4.5, 3 / 5]) and np.allclose(m.precision, [1 / 1.5, 1.0])
    assert np.allclose(m.tp_rates, [1.0, 0.5]) and np.allclose(m.fp_rates, [0.5 / 3.5, 0.0])


# ---- ValidateCallback ----------------------------------------------------------------------------------------------------------
class _Statistic:
    calls = []

    def __init__(self, embeddings, labels, config):
        self.dict = {"n": len(labels), "metric": config.metric, "sum": float(np.sum(embeddings))}
        _Statistic.calls.append(self.dict)

    def __repr__(self):
        return "stub report {}\n".format(self.dict["n"])

    def write_report(self, file):
        with open(file, "at") as f:
            f.write(repr(self))


class _Model:
    def __init__(self, path=None):
        self.path, self.seen = path, 0

    def __call__(self, images):
        self.seen += len(images)
        return np.asarray(images, dtype=np.float32).reshape(len(images), -1)[:, :2]


_VALIDATE = Config({"validate": {"metric": 1, "nrof_folds": 2, "far_target": 1e-3}})


@pytest.mark.parametrize("every,last", [(1, 4), (3, 7), (3, 8), (10, 25), (10, 7)])
def test_epoch_rule(every, last):
    due = [e + 1 for e in range(last) if callbacks.validation_due(e, every, last)]
    assert due == sorted(set(range(every, last + 1, every)) | {last})
    data = [(np.ones((3, 2, 2, 3), np.uint8), np.arange(3))]
    cb = callbacks.ValidateCallback(_Model(), data, every, last, _VALIDATE, log=lambda *_: None, statistic=_Statistic)
    for e in range(last):
        cb.on_epoch_end(e)
    assert [h[0] for h in cb.history] == due


def test_every_n_epochs_below_one_raises():
    for bad in (0, -2, None):
        with pytest.raises(ValueError):
            callbacks.ValidateCallback(_Model(), [], bad, 10, _VALIDATE)


def test_history_and_report_file(tmp_path):
    data = [(np.full((4, 2, 2, 3), 1, np.uint8), np.array([0, 0, 1, 1])), (np.full((3, 2, 2, 3), 2, np.uint8), np.array([1, 2, 2]))]
    model = _Model(path=tmp_path / "run")
    lines = []
    cb = callbacks.ValidateCallback(model, data, 2, 3, _VALIDATE, log=lambda s: lines.append(str(s)), statistic=_Statistic)
    for e in range(3):
        cb.on_epoch_end(e)
    assert [h[0] for h in cb.history] == [2, 3] and model.seen == 14
    for epoch1, d, t_embed, t_stat in cb.history:
        assert d == {"n": 7, "metric": 1, "sum": 4 * 2 * 1.0 + 3 * 2 * 2.0} and t_embed >= 0 and t_stat >= 0
    assert np.array_equal(cb.labels, [0, 0, 1, 1, 1, 2, 2]) and cb.embeddings.shape == (7, 2)
    assert (tmp_path / "run" / "report.txt").read_text() == "stub report 7\n" * 2
    assert "perform validation for epoch 2" in lines and "stub report 7\n" in lines
    # the decoded batches are kept after the first pass; above the limit every pass walks the data set again
    assert cb._resident is not None and len(cb._resident) == 2
    small = callbacks.ValidateCallback(_Model(), data, 1, 1, _VALIDATE, log=lambda *_: None, statistic=_Statistic, resident_bytes=50)
    small.on_epoch_end(0)
    assert small._resident is None and small.history[0][1]["n"] == 7
    assert callbacks.RESIDENT_BYTES == 4 << 30
    # no model.path: nothing is written
    nowhere = callbacks.ValidateCallback(_Model(), data, 1, 1, _VALIDATE, log=lambda *_: None, statistic=_Statistic)
    nowhere.on_epoch_end(0)
    assert len(nowhere.history) == 1


@pytest.mark.parametrize("world", [1, 2, 3])
def test_rank_sharding_and_reordering(world):
    n, batch = 23, 4                                  # 6 batches, the last one short; not a multiple of batch x world
    rows = np.arange(n * 2, dtype=np.float32).reshape(n, 2)
    data = [(rows[i:i + batch], np.arange(i, min(i + batch, n))) for i in range(0, n, batch)]
    per_rank_e, per_rank_l = [], []
    for rank in range(world):
        cb = callbacks.ValidateCallback(lambda x: x, data, 1, 1, _VALIDATE, rank=rank, world=world)
        mine = list(cb._batches())
        assert [int(l[0]) // batch for _, l in mine] == callbacks.shard(len(data), rank, world)
        per_rank_e.append([np.asarray(x) for x, _ in mine])
        per_rank_l.append([l for _, l in mine])
    assert np.array_equal(np.concatenate(callbacks.interleave(per_rank_e)), rows)
    assert np.array_equal(np.concatenate(callbacks.interleave(per_rank_l)), np.arange(n))
    if world > 1:
        with pytest.raises(ValueError):
            callbacks.interleave([per_rank_e[0][:-1]] + per_rank_e[1:])


# ---- configuration --------------------------------------------------------------------------------------------------------------
def test_validate_defaults_and_no_callback_without_a_path():
    cfg = load_config()
    assert cfg.validate.as_dict == {
        "every_n_epochs": 10, "averaged": False,
        "dataset": {"path": None, "h5file": None, "nrof_classes": None, "min_nrof_images": None, "max_nrof_images": 50},
        "validate": {"metric": 0, "nrof_folds": 10, "far_target": 0.001}}
    assert callbacks.from_config(cfg) is None
    cfg = load_config(overrides={"validate": {"every_n_epochs": 5}})
    assert cfg.validate.every_n_epochs == 5 and cfg.validate.validate.nrof_folds == 10 and callbacks.from_config(cfg) is None


def test_validate_app_options(tmp_path):
    from facenet_amd.apps.validate import load_options
    model_dir = tmp_path / "20200724-231357"
    model_dir.mkdir()
    opt = load_options(overrides={"model": {"path": str(model_dir), "normalize": False}})
    assert opt.model.normalize is True and opt.file == model_dir / "report.txt"
    assert opt.validate.as_dict == {"nrof_folds": 10, "metric": 0, "far_target": 0.001}
    weights = model_dir / "weights.npz"
    assert load_options(overrides={"model": {"path": str(weights)}}).file == model_dir / "report.txt"
    assert load_options(overrides={"file": str(tmp_path / "out.txt")}).file == tmp_path / "out.txt"
    yaml_file = tmp_path / "validate.yaml"
    yaml_file.write_text("validate:\n  metric: 1\nmodel:\n  path: {}\n".format(model_dir))
    opt = load_options(yaml_file)
    assert opt.validate.metric == 1 and opt.validate.nrof_folds == 10 and opt.model.normalize is True
