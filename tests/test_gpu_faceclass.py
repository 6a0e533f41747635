"""Pair classifiers on the GPU (oracle: tests/faceclass_oracle.py): the loss and gradient kernel, the
distance and count kernels, Adam over several steps, graph replay, ConfusionMatrix and both apps."""
import random

import numpy as np
import pytest
import torch

from facenet_amd import _lib
from facenet_amd.apps import train_classifier as app
from facenet_amd.config import Config
from facenet_amd.faceclass import (ClassifierTrainer, FaceToFaceDistanceClassifier, FaceToFaceNormalizedEmbeddingsClassifier,
                                   pos_weight, row_norms)
from facenet_amd.facenet import equal_batches_input_pipeline
from tests import faceclass_oracle as fo
from tests.util import ptr, stream

pytestmark = pytest.mark.gpu

MODES = [fo.MODE_DISTANCE, fo.MODE_NORMALIZED]


def _model(mode, values=(7.0, 1.1, 0.8)):
    m = FaceToFaceDistanceClassifier() if mode == fo.MODE_DISTANCE else FaceToFaceNormalizedEmbeddingsClassifier()
    m.params[:3] = torch.tensor(values)
    return m


def _classes(sizes, E, seed, mode):
    embs = fo.clustered(sizes, E, seed)
    if mode == fo.MODE_NORMALIZED:
        embs = [(e / np.linalg.norm(e, axis=1, keepdims=True)).astype(np.float32) for e in embs]
    return embs


def _loss_launch(tr):
    """The loss kernel alone on the trainer's buffers: (loss, grad) as numpy."""
    lib = _lib.load()
    _lib.check(lib.fn_f2f_pair_loss_fwd_bwd(ptr(tr.table), ptr(tr.norms) if tr.norms is not None else None, tr.n_rows, ptr(tr.rows), tr.P,
                                            tr.K, tr.E, tr.model.mode, tr.q, ptr(tr.model.params), ptr(tr.loss), ptr(tr.grad), ptr(tr.ws),
                                            tr.ws.numel(), stream()))
    torch.cuda.synchronize()
    return tr.loss.cpu().numpy().copy(), tr.grad.cpu().numpy().copy()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("P,K,E", [(1, 3, 128), (7, 3, 128), (50, 5, 512), (500, 5, 512)])
def test_loss_and_gradients_match_the_oracle(mode, P, K, E):
    embs = _classes([K + 3] * max(P, 2), E, seed=P * 7 + K, mode=mode)
    m = _model(mode)
    tr = ClassifierTrainer(m, embs, P, K)
    random.seed(P + K)
    rows = next(equal_batches_input_pipeline(embs, Config({"nrof_classes_per_batch": P, "nrof_examples_per_class": K})))
    tr.set_rows(rows)
    loss, grad = _loss_launch(tr)
    batch = np.concatenate(embs)[rows]
    want_loss, want_grad, scale = fo.pair_loss(batch, P, K, mode, 7.0, 1.1, 0.8)
    assert tr.q == fo.pos_weight(P, K) if P * K <= 350 else tr.q == pos_weight(P, K)
    assert abs(loss[0] - want_loss) <= 1e-4 * abs(want_loss), (loss[0], want_loss)
    # relative to the size of the summed terms: a gradient that nearly cancels is checked against its terms' scale
    for j in range(3):
        assert abs(grad[j] - want_grad[j]) <= 1e-4 * max(abs(want_grad[j]), scale[j] * 1e-2) + 1e-12, (j, grad[j], want_grad[j])
    assert grad[3] == 0.0
    if mode == fo.MODE_NORMALIZED:
        assert grad[2] == 0.0


@pytest.mark.parametrize("mode", MODES)
def test_two_launches_are_bitwise_equal_and_nan_propagates(mode):
    P, K, E = 50, 5, 512
    embs = _classes([8] * P, E, seed=1, mode=mode)
    tr = ClassifierTrainer(_model(mode), embs, P, K)
    random.seed(0)
    rows = next(equal_batches_input_pipeline(embs, Config({"nrof_classes_per_batch": P, "nrof_examples_per_class": K})))
    tr.set_rows(rows)
    a, b = _loss_launch(tr), _loss_launch(tr)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    tr.table[int(rows[17]), 5] = float("nan")
    if tr.norms is not None:
        tr.norms.copy_(row_norms(tr.table))
    loss, grad = _loss_launch(tr)
    assert np.isnan(loss[0])
    assert np.all(np.isnan(grad[:3 if mode == fo.MODE_DISTANCE else 2]))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("N,M,E", [(37, 70, 128), (130, 65, 512)])
def test_distance_and_logits_match_the_oracle(mode, N, M, E):
    x = np.concatenate(_classes([N], E, seed=N, mode=mode))
    y = np.concatenate(_classes([M], E, seed=M, mode=mode))
    m = _model(mode)
    theta = 0.8 if mode == fo.MODE_DISTANCE else 1.0
    want = fo.distance(x, y, mode, theta)
    got = m.distance(x, y)
    assert isinstance(got, np.ndarray) and got.shape == (N, M)
    assert np.max(np.abs(got - want)) <= 2e-6
    # y = x: rows of one cluster are nearly parallel, their dot sums to ~|x|^2 in one 512-long fp32 chain
    np.testing.assert_allclose(m.distance(x), fo.distance(x, None, mode, theta), rtol=0, atol=4e-6)
    lg = m(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda())
    assert torch.is_tensor(lg) and lg.is_cuda
    np.testing.assert_allclose(lg.cpu().numpy(), fo.logits(x, y, mode, 7.0, 1.1, theta), rtol=0, atol=2e-5)
    assert np.array_equal(m.predict(x, y), got < np.float32(1.1))


@pytest.mark.parametrize("mode", MODES)
def test_counts_equal_distance_below_threshold_on_ragged_classes(mode):
    rng = np.random.default_rng(5)
    sizes = list(rng.integers(1, 61, 40))
    sizes[0], sizes[1] = 1, 60
    embs = _classes(sizes, 128, seed=9, mode=mode)
    m = _model(mode, (10.0, 1.0, 1.0))
    table = torch.from_numpy(np.concatenate(embs)).cuda()
    counts = app.pair_counts(embs, m)
    starts = np.concatenate([[0], np.cumsum(sizes)])
    below = (m.distance(table) < m.params[1]).cpu().numpy()
    C = len(sizes)
    ambiguous = 0
    for i in range(C):
        for k in range(i + 1):
            blk = below[starts[i]:starts[i + 1], starts[k]:starts[k + 1]]
            assert counts[i * (i + 1) // 2 + k] == blk.sum(), (i, k)
            d64 = fo.distance(embs[i], embs[k], mode, 1.0)
            near = np.abs(d64 - 1.0) < 1e-5
            ambiguous += near.sum()
            assert abs(int(counts[i * (i + 1) // 2 + k]) - int((d64 < 1.0).sum())) <= near.sum(), (i, k)
    # 2x: the square blocks hold both orders of a pair
    assert counts.sum() > 0 and ambiguous <= 2 * len(below) ** 2


def test_threshold_change_on_device_changes_the_counts():
    embs = _classes([20] * 12, 128, seed=3, mode=fo.MODE_DISTANCE)
    m = _model(fo.MODE_DISTANCE, (10.0, 1.0, 1.0))
    addr = m.params.data_ptr()
    before = app.pair_counts(embs, m)
    m.params[1] = 1.6
    after = app.pair_counts(embs, m)
    assert m.params.data_ptr() == addr
    assert after.sum() > before.sum()
    d = [fo.distance(embs[i], embs[k], 0, 1.0) for i in range(12) for k in range(i + 1)]
    np.testing.assert_array_equal(after, [int((x < 1.6).sum()) for x in d])


@pytest.mark.parametrize("mode", MODES)
def test_adam_trajectory_with_stepped_learning_rate(mode):
    P, K, E = 7, 3, 128
    embs = _classes([6] * 10, E, seed=11, mode=mode)
    m = _model(mode, (10.0, 1.0, 1.0))
    tr = ClassifierTrainer(m, embs, P, K, learning_rate=0.05)
    table = np.concatenate(embs)
    random.seed(2)
    gen = equal_batches_input_pipeline(embs, Config({"nrof_classes_per_batch": P, "nrof_examples_per_class": K}))
    w, mm, vv = np.array([10.0, 1.0, 1.0]), np.zeros(3), np.zeros(3)
    for t in range(20):
        lr = fo.learning_rate(0.05, 0.5, 5, t)
        tr.set_learning_rate(lr)
        rows = next(gen)
        tr.step(rows)
        want_loss, g, _ = fo.pair_loss(table[rows], P, K, mode, *w)
        w, mm, vv = fo.adam(w, g, mm, vv, t + 1, np.float32(lr))
        got = m.params.cpu().numpy()[:3].astype(np.float64)
        np.testing.assert_allclose(got, w, rtol=1e-4)
        assert tr.loss_value() == pytest.approx(want_loss, rel=1e-4)
    assert tr.global_step == 20


@pytest.mark.parametrize("mode", MODES)
def test_captured_replay_equals_eager_steps(mode):
    P, K, E = 50, 5, 512
    embs = _classes([7] * 60, E, seed=4, mode=mode)
    runs = []
    for captured in (False, True):
        m = _model(mode, (10.0, 1.0, 1.0))
        tr = ClassifierTrainer(m, embs, P, K, learning_rate=0.01)
        if captured:
            tr.capture()
        random.seed(8)
        gen = equal_batches_input_pipeline(embs, Config({"nrof_classes_per_batch": P, "nrof_examples_per_class": K}))
        for t in range(6):
            if t == 3:
                tr.set_learning_rate(0.001)
            tr.step(next(gen))
        torch.cuda.synchronize()
        runs.append([x.cpu().numpy().tobytes() for x in (m.params, tr.M, tr.V, tr.loss, tr.hyper)])
    assert runs[0] == runs[1]


@pytest.mark.parametrize("mode", MODES)
def test_confusion_matrix_matches_the_oracle(mode):
    sizes = [3, 9, 5, 7, 4, 8, 6, 5, 9, 3, 7, 6]
    embs = _classes(sizes, 64, seed=21, mode=mode)
    m = _model(mode, (10.0, 1.0, 1.0))
    d = [fo.distance(embs[i], embs[k], mode, 1.0) for i in range(len(sizes)) for k in range(i + 1)]
    assert min(np.min(np.abs(x - 1.0)) for x in d) > 1e-4          # no pair on the threshold: the counts are exact
    cm = app.ConfusionMatrix(embs, m)
    want = fo.confusion_matrix(embs, mode, 1.0, 1.0)
    for key, v in want.items():
        assert getattr(cm, key) == pytest.approx(v, rel=1e-12, abs=1e-15), key
    text = repr(cm)
    assert text.startswith("ConfusionMatrix\n") and "accuracy  " in text and "tn rate   " in text
    assert "variables {'alpha': 10.0, 'threshold': 1.0" in text


@pytest.mark.parametrize("normalize", [False, True])
def test_train_classifier_app_end_to_end(tmp_path, normalize):
    embs = fo.clustered([8] * 6, 32, seed=13)
    labels = np.concatenate([np.full(8, c + 100) for c in range(6)])
    f = tmp_path / "emb.npz"
    np.savez(f, embeddings=np.concatenate(embs), labels=labels)
    opts = app.load_options(overrides={
        "nrof_classes_per_batch": 3, "nrof_examples_per_class": 4, "classifier": {"path": str(tmp_path / "cls")},
        "train": {"epoch": {"max_nrof_epochs": 2, "size": 5}},
        "embeddings": {"path": str(f), "max_nrof_images": 50, "normalize": normalize}})
    lines = []
    model, tr = app.train_classifier(opts, log=lambda s: lines.append(str(s)))
    assert tr.global_step == 10
    log = opts.logfile.read_text()
    assert "epoch [1/2], learning rate 0.01," in log and "epoch [2/2], learning rate 0.001" in log and log.count("ConfusionMatrix") == 2
    saved = opts.classifier.path / "classifier.npz"
    cls = FaceToFaceNormalizedEmbeddingsClassifier if normalize else FaceToFaceDistanceClassifier
    back = cls().load(saved)
    assert torch.equal(back.params[:len(cls.names)].cpu(), model.params[:len(cls.names)].cpu())
    with np.load(saved) as z:
        assert sorted(z.files) == sorted(f"{n}:0" for n in cls.names)


def test_embeddings_app_end_to_end(tmp_path):
    from PIL import Image

    from facenet_amd.apps import embeddings as emb_app
    from facenet_amd.facenet import Embeddings

    rng = np.random.default_rng(0)
    for c in range(2):
        d = tmp_path / "data" / f"person_{c}"
        d.mkdir(parents=True)
        for i in range(3):
            Image.fromarray(rng.integers(0, 256, (160, 160, 3), dtype=np.uint8)).save(d / f"img_{i}.png")
    out = tmp_path / "out" / "embeddings.npz"
    opts = emb_app.load_options(overrides={"dataset": {"path": str(tmp_path / "data")}, "outfile": str(out), "batch_size": 4,
                                           "model": {"embedding_size": 128}})
    emb_app.write_embeddings(opts, log=lambda s: None)
    with np.load(out) as z:
        assert z["embeddings"].shape == (6, 128) and z["embeddings"].dtype == np.float32
        np.testing.assert_array_equal(z["labels"], [0, 0, 0, 1, 1, 1])
        assert len(z["files"]) == 6 and np.all(np.isfinite(z["embeddings"]))
    e = Embeddings(Config({"path": str(out)}))
    assert e.nrof_classes == 2 and e.length == 128
    assert (tmp_path / "out" / "log.txt").exists()
