"""CPU checks of the pair classifiers: the oracle's analytic gradients and loss form, pos_weight, the
equal-batches sampler against the reference generator, Embeddings subsampling, the argument errors, and the new C ABI
symbols."""
import random
import re
from pathlib import Path

import numpy as np
import pytest

from facenet_amd import _lib, faceclass
from facenet_amd.apps import embeddings as embeddings_app
from facenet_amd.apps import train_classifier as app
from facenet_amd.config import Config
from facenet_amd.facenet import Embeddings, equal_batches_input_pipeline, split_embeddings
from tests import faceclass_oracle as fo

ROOT = Path(__file__).resolve().parents[1]
NEW_SYMBOLS = ["fn_f2f_row_norms", "fn_f2f_pair_loss_fwd_bwd", "fn_f2f_pair_counts", "fn_f2f_distance"]


def test_new_symbols_are_declared_and_exported():
    header = (ROOT / "include" / "facenet_hip.h").read_text()
    for name in NEW_SYMBOLS:
        assert re.search(rf"\bint {name}\(", header), name
        assert name in _lib.EXPORTS, name


@pytest.mark.parametrize("mode", [fo.MODE_DISTANCE, fo.MODE_NORMALIZED])
def test_oracle_gradients_match_central_differences(mode):
    P, K, E = 3, 3, 8
    batch = np.concatenate(fo.clustered([K] * P, E, seed=mode + 1, dtype=np.float64))
    if mode == fo.MODE_NORMALIZED:
        batch /= np.linalg.norm(batch, axis=1, keepdims=True)
    v = np.array([7.0, 1.1, 0.8])
    _, grads, _ = fo.pair_loss(batch, P, K, mode, *v)
    h = 1e-6
    for j in range(3 if mode == fo.MODE_DISTANCE else 2):
        e = np.zeros(3)
        e[j] = h
        num = (fo.pair_loss(batch, P, K, mode, *(v + e))[0] - fo.pair_loss(batch, P, K, mode, *(v - e))[0]) / (2 * h)
        assert abs(num - grads[j]) <= 1e-6 * max(1.0, abs(num)), (j, num, grads[j])
    if mode == fo.MODE_NORMALIZED:
        assert grads[2] == 0.0


def test_weighted_bce_form():
    rng = np.random.default_rng(3)
    s = rng.standard_normal(200) * 6
    z = (rng.random(200) < 0.3).astype(np.float64)
    for q in (0.0, 0.5, 3.0, 24.0):
        sig = 1 / (1 + np.exp(-s))
        plain = -(q * z * np.log(sig) + (1 - z) * np.log(1 - sig))
        np.testing.assert_allclose(fo.weighted_bce(z, s, q), plain, rtol=1e-7, atol=1e-12)   # the plain form cancels for large |s|


@pytest.mark.parametrize("P,K", [(1, 2), (1, 5), (2, 2), (7, 3), (50, 5), (500, 5)])
def test_pos_weight(P, K):
    want = (P * K * (P * K - 1) / 2) / (P * K * (K - 1) / 2) - 1
    assert faceclass.pos_weight(P, K) == want
    if P * K <= 350:
        assert faceclass.pos_weight(P, K) == pytest.approx(fo.pos_weight(P, K), rel=1e-15)
    if P == 1:
        assert faceclass.pos_weight(P, K) == 0.0


@pytest.mark.parametrize("P,K", [(3, 2), (5, 4), (8, 3)])
def test_sampler_picks_the_reference_rows(P, K):
    embs = fo.clustered([4, 9, 5, 7, 6, 8, 4, 10], 4, seed=5)
    table = np.concatenate(embs)
    random.seed(11)
    ref = fo.reference_batches(embs, P, K)
    want = [np.asarray(next(ref), np.float32) for _ in range(6)]
    random.seed(11)
    gen = equal_batches_input_pipeline(embs, Config({"nrof_classes_per_batch": P, "nrof_examples_per_class": K}))
    for w in want:
        rows = next(gen)
        assert rows.dtype == np.int32 and rows.shape == (P * K,)
        np.testing.assert_array_equal(table[rows], w)


def test_sampler_defaults_are_written_back():
    embs = fo.clustered([20, 30, 40], 4, seed=1)
    cfg = Config({"nrof_classes_per_batch": None, "nrof_examples_per_class": None})
    equal_batches_input_pipeline(embs, cfg)
    assert cfg.nrof_classes_per_batch == 3 and cfg.nrof_examples_per_class == 3     # round(0.1 * 90 / 3)


def _write_npz(path, embs):
    labels = np.concatenate([np.full(len(e), 10 * c) for c, e in enumerate(embs)])
    x = np.concatenate(embs)
    order = np.random.default_rng(0).permutation(len(x))
    np.savez(path, embeddings=x[order], labels=labels[order])


def test_embeddings_subsampling_and_normalisation(tmp_path):
    embs = fo.clustered([12, 3, 7, 20, 9, 15], 8, seed=2)
    f = tmp_path / "emb.npz"
    _write_npz(f, embs)
    with np.load(f) as d:
        split = split_embeddings(d["embeddings"], d["labels"])
    random.seed(4)
    want = fo.reference_subsample(list(split), 4, 8)
    random.seed(4)
    e = Embeddings(Config({"path": str(f), "nrof_classes": 4, "max_nrof_images": 8}))
    assert e.nrof_classes == 4 and e.length == 8 and e.nrof_images == sum(len(w) for w in want)
    for got, w in zip(e.data(), want):
        np.testing.assert_array_equal(got, w)
    normed = e.data(normalize=True)
    for got, w in zip(normed, want):
        np.testing.assert_allclose(np.linalg.norm(got, axis=1), 1.0, rtol=1e-6)
        np.testing.assert_allclose(got, w / np.linalg.norm(w, axis=1, keepdims=True), rtol=1e-6)
    assert "Number of classes 4" in repr(e)


def test_errors():
    embs = fo.clustered([4, 5, 3], 4, seed=0)
    with pytest.raises(ValueError, match="at least 2"):
        equal_batches_input_pipeline(embs, Config({"nrof_classes_per_batch": 2, "nrof_examples_per_class": 1}))
    with pytest.raises(ValueError, match="fewer than"):
        equal_batches_input_pipeline(embs, Config({"nrof_classes_per_batch": 2, "nrof_examples_per_class": 4}))
    with pytest.raises(ValueError, match="at least 2 classes"):
        app.ConfusionMatrix(embs[:1], object())
    with pytest.raises(ValueError, match="h5py"):
        Embeddings(Config({"path": "/nonexistent/embeddings.h5"}))
    with pytest.raises(ValueError, match="ADAM"):
        faceclass.check_optimizer("MOM")
    with pytest.raises(ValueError, match="ADAM"):
        faceclass.ClassifierTrainer(object(), embs, 2, 2, optimizer="RMSPROP")
    with pytest.raises(ValueError, match="ADAM"):
        app.train_classifier(app.load_options(overrides={"train": {"optimizer": "ADAGRAD"}, "classifier": {"path": "/nonexistent"}}))
    for suffix in (".h5", ".tfrecord"):
        with pytest.raises(ValueError):
            embeddings_app.load_options(overrides={"outfile": f"/nonexistent/embeddings{suffix}"})


def test_learning_rate_schedule():
    sched = Config({"initial_value": 0.01, "decay_rate": 0.1, "decay_steps": None})
    for step in (0, 1, 249, 250, 499, 500, 1234):
        assert app.learning_rate(sched, 250, step) == pytest.approx(fo.learning_rate(0.01, 0.1, 250, step), rel=1e-15)
    sched.decay_steps = 7
    assert app.learning_rate(sched, 250, 14) == pytest.approx(0.01 * 0.1 ** 2, rel=1e-15)
