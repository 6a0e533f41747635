# coding:utf-8
"""Face-to-face pair classifiers of facenet/faceclass.py:8-118 on the HIP path, and their trainer.

``FaceToFaceDistanceClassifier`` and ``FaceToFaceNormalizedEmbeddingsClassifier`` decide "same person?" from a distance
between two embeddings: ``logits = alpha (threshold - d)``, ``predict = d < threshold``.  Their variables live in one device
word ``params`` = fp32[4] {alpha, threshold, theta, 0} that the kernels read on the device, so a captured training step sees
the optimiser's updates.  ``distance`` / ``__call__`` / ``predict`` run fn_f2f_distance: NumPy in gives NumPy out, a device
tensor in gives a device tensor out.

``ClassifierTrainer`` is the training step of apps/train_classifier.py:60-135: the class-weighted
binary cross-entropy over every pair of a class-grouped batch (fn_f2f_pair_loss_fwd_bwd) followed by Adam (fn_adam_tick +
fn_adam_keras), eagerly or replayed from a captured HIP graph."""
from __future__ import annotations

from pathlib import Path

import numpy as np
import torch

from . import _lib
from ._call import as_table, ptr, stream

MODE_DISTANCE, MODE_NORMALIZED = 0, 1
TILE = 64                 # rows per tile side of fn_f2f_pair_loss_fwd_bwd (include/facenet_hip.h)
ADAM_BETA1, ADAM_BETA2, ADAM_EPSILON = 0.9, 0.999, 0.1


def row_norms(table: torch.Tensor) -> torch.Tensor:
    """|x_r| of every row (fn_f2f_row_norms)."""
    out = torch.empty(table.shape[0], dtype=torch.float32, device=table.device)
    _lib.check(_lib.load().fn_f2f_row_norms(ptr(table), table.shape[0], table.shape[1], ptr(out), stream(table.device)),
               "f2f_row_norms")
    return out


class _FaceToFaceClassifier:
    mode = MODE_DISTANCE
    names = ("alpha", "threshold", "theta")
    _SLOT = {"alpha": 0, "threshold": 1, "theta": 2}

    def __init__(self, device="cuda"):
        self.device = torch.device(device)
        # alpha = 10, threshold = 1, theta = 1 (faceclass.py:18-22, :86-89); the pad word stays 0
        self.params = torch.tensor([10.0, 1.0, 1.0, 0.0], dtype=torch.float32, device=self.device)

    @property
    def variables(self):
        """name -> 0-d view of the device word (the reference's tf.Variables)."""
        return {name: self.params[self._SLOT[name]] for name in self.names}

    def variable(self, name, mode=None):
        var = self.variables[name]
        if mode == "numpy":
            return np.float32(var.item())
        return var

    def __repr__(self):
        variables = {name: float(self.variable(name, mode="numpy")) for name in self.names}
        return (f"{self.__class__.__name__}\n"
                f"variables {variables}\n")

    def _matrix(self, x, y, logits):
        numpy_in = not torch.is_tensor(x)
        xt = as_table(x, self.device)
        yt = xt if y is None else as_table(y, self.device)
        if yt.shape[1] != xt.shape[1]:
            raise ValueError(f"embedding lengths differ: {xt.shape[1]} and {yt.shape[1]}")
        nx = ny = None
        if self.mode == MODE_DISTANCE:
            nx = row_norms(xt)
            ny = nx if y is None else row_norms(yt)
        out = torch.empty(xt.shape[0], yt.shape[0], dtype=torch.float32, device=self.device)
        _lib.check(_lib.load().fn_f2f_distance(ptr(xt), ptr(nx), xt.shape[0], ptr(yt), ptr(ny), yt.shape[0], xt.shape[1], self.mode,
                                               ptr(self.params), int(logits), ptr(out), stream(self.device)), "f2f_distance")
        return out.cpu().numpy() if numpy_in else out

    def __call__(self, x, y=None):
        """logits = alpha (threshold - d(x, y)) (faceclass.py:23-27)."""
        return self._matrix(x, y, logits=True)

    def distance(self, x, y=None):
        return self._matrix(x, y, logits=False)

    def predict(self, x, y=None):
        """d(x, y) < threshold (faceclass.py:79-80)."""
        d = self.distance(x, y)
        if torch.is_tensor(d):
            return d < self.params[1]
        return d < self.variable("threshold", mode="numpy")

    def save(self, path):
        """.npz with one key per variable, TF-style names ('alpha:0', ...)."""
        np.savez(path, **{f"{name}:0": self.variable(name, mode="numpy") for name in self.names})

    def load(self, path):
        with np.load(path) as f:
            for name in self.names:
                self.params[self._SLOT[name]] = float(f[f"{name}:0"])
        return self


class FaceToFaceDistanceClassifier(_FaceToFaceClassifier):
    """faceclass.py:8-80: d = 2 (1 - x1.y1) + theta (2 (|x| - |y|) / (|x| + |y|))^2 with x1 = x / |x|, y1 = y / |y|."""
    mode = MODE_DISTANCE
    names = ("alpha", "threshold", "theta")


class FaceToFaceNormalizedEmbeddingsClassifier(_FaceToFaceClassifier):
    """faceclass.py:83-118: d = 2 (1 - x.y) on embeddings normalised beforehand (Embeddings.data(normalize=True))."""
    mode = MODE_NORMALIZED
    names = ("alpha", "threshold")


def pos_weight(P: int, K: int) -> float:
    """train_classifier.py:74: #pairs / #positive pairs - 1, in float64 (0 for a single class)."""
    B = P * K
    return (B * (B - 1) / 2) / (P * K * (K - 1) / 2) - 1


def check_optimizer(name):
    """Only Adam is defined (the reference's facenet.train_op no longer exists)."""
    if name != "ADAM":
        raise ValueError(f"Invalid optimization algorithm {name!r}: only ADAM is supported")


class ClassifierTrainer:
    """One training step on a resident class-grouped table: rows -> loss and gradient -> Adam on the classifier's params.

    ``embeddings`` is the list of per-class arrays of Embeddings.data(); a batch is an int32 array of P K row indices into
    their concatenation, grouped by class (equal_batches_input_pipeline).  Adam: beta1 0.9, beta2 0.999, epsilon 0.1, no L2
    (the update of TF1's AdamOptimizer); the learning rate is a device word set with ``set_learning_rate``."""

    def __init__(self, model: _FaceToFaceClassifier, embeddings, nrof_classes_per_batch: int, nrof_examples_per_class: int,
                 learning_rate: float = 0.01, optimizer: str = "ADAM"):
        check_optimizer(optimizer)
        P, K = int(nrof_classes_per_batch), int(nrof_examples_per_class)
        if K < 2:
            raise ValueError(f"nrof_examples_per_class must be at least 2, got {K}")
        if P < 1:
            raise ValueError(f"nrof_classes_per_batch must be at least 1, got {P}")
        self.model, self.P, self.K, self.B = model, P, K, P * K
        dev = self.device = model.device
        arrays = list(embeddings) if isinstance(embeddings, (list, tuple)) else [embeddings]
        self.table = as_table(np.concatenate([np.asarray(e, dtype=np.float32) for e in arrays]) if not torch.is_tensor(arrays[0])
                               else torch.cat(arrays), dev)
        self.n_rows, self.E = self.table.shape
        self.norms = row_norms(self.table) if model.mode == MODE_DISTANCE else None
        self.q = pos_weight(P, K)
        nt = -(-self.B // TILE)
        self.ws = torch.zeros(4 * (nt * (nt + 1) // 2), dtype=torch.float64, device=dev)
        self.rows = torch.zeros(self.B, dtype=torch.int32, device=dev)
        self.loss = torch.zeros(1, dtype=torch.float32, device=dev)
        self.grad = torch.zeros(4, dtype=torch.float32, device=dev)
        self.M = torch.zeros(4, dtype=torch.float32, device=dev)
        self.V = torch.zeros(4, dtype=torch.float32, device=dev)
        # {lr, beta1^t, beta2^t, grad_scale, t (int32 bits), 3 spare}: the hyper words of fn_adam_keras / fn_adam_tick
        self.hyper = torch.tensor([learning_rate, 1.0, 1.0, 1.0, 0.0, 0.0, 0.0, 0.0], dtype=torch.float32, device=dev)
        self._graph = None

    def _launch(self):
        lib, st = _lib.load(), stream(self.device)
        _lib.check(lib.fn_f2f_pair_loss_fwd_bwd(ptr(self.table), ptr(self.norms), self.n_rows, ptr(self.rows), self.P, self.K, self.E,
                                                self.model.mode, self.q, ptr(self.model.params), ptr(self.loss), ptr(self.grad),
                                                ptr(self.ws), self.ws.numel(), st), "f2f_pair_loss_fwd_bwd")
        _lib.check(lib.fn_adam_tick(ptr(self.hyper), ADAM_BETA1, ADAM_BETA2, st), "adam_tick")
        _lib.check(lib.fn_adam_keras(ptr(self.model.params), ptr(self.grad), ptr(self.M), ptr(self.V), None, 0, 4, 0, ptr(self.hyper),
                                     ADAM_BETA1, ADAM_BETA2, ADAM_EPSILON, 0.0, _lib.FN_BF16, st), "adam_keras")

    def set_rows(self, rows):
        rows = np.asarray(rows)
        if rows.shape != (self.B,):
            raise ValueError(f"a batch holds {self.B} row indices, got shape {rows.shape}")
        if rows.min() < 0 or rows.max() >= self.n_rows:
            raise ValueError(f"row index outside [0, {self.n_rows})")
        self.rows.copy_(torch.from_numpy(rows.astype(np.int32)))

    def step(self, rows=None):
        """One step on the batch ``rows`` (or on the rows already resident)."""
        if rows is not None:
            self.set_rows(rows)
        if self._graph is None:
            self._launch()
        else:
            self._graph.replay()

    def capture(self):
        """Capture the step into a HIP graph.  Side-effect free: the warm-up step's changes to the parameters, the Adam slots
        and the step count are undone, so capture() followed by n steps equals n eager steps."""
        state = (self.model.params, self.M, self.V, self.hyper, self.loss, self.grad)
        saved = [t.clone() for t in state]
        self._launch()
        torch.cuda.synchronize(self.device)
        for t, s in zip(state, saved):
            t.copy_(s)
        torch.cuda.synchronize(self.device)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self._launch()
        self._graph = g

    def set_learning_rate(self, lr: float):
        self.hyper[0:1].fill_(float(lr))        # device write: the next replay reads it

    @property
    def global_step(self) -> int:
        return int(self.hyper.view(torch.int32)[4].item())

    def loss_value(self) -> float:
        return float(self.loss.item())
