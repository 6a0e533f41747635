# coding:utf-8
"""Train a face-to-face pair classifier on an embeddings file, as apps/train_classifier.py:17-135 of the reference:
``python -m facenet_amd.apps.train_classifier --config x.yaml``.

Embeddings (an .npz of facenet_amd.apps.embeddings) -> per-class arrays -> equal batches of P classes x K rows ->
FaceToFaceDistanceClassifier (or FaceToFaceNormalizedEmbeddingsClassifier with ``embeddings.normalize``) trained with the
class-weighted binary cross-entropy over every pair of the batch and Adam, ``train.epoch.max_nrof_epochs`` x
``train.epoch.size`` steps replayed from a captured HIP graph.  After every epoch the ConfusionMatrix over all classes;
``log.txt`` and ``classifier.npz`` are written under ``classifier.path``/<timestamp>.  Semantics: DESIGN.md section 12."""
from __future__ import annotations

import math
import random
from datetime import datetime
from pathlib import Path

import click
import numpy as np
import torch

from facenet_amd import _lib
from facenet_amd._call import as_table, ptr, stream
from facenet_amd.config import Config, _merge
from facenet_amd.faceclass import (ClassifierTrainer, FaceToFaceDistanceClassifier, FaceToFaceNormalizedEmbeddingsClassifier,
                                   check_optimizer, row_norms)
from facenet_amd.facenet import Embeddings, equal_batches_input_pipeline

# apps/configs/train_classifier.yaml of the reference (embeddings.path names an .npz here) and config.yaml's seed
DEFAULTS = {
    "seed": 0,
    "nrof_classes_per_batch": None,
    "nrof_examples_per_class": 5,
    "classifier": {"path": "~/models/facenet/classifier"},
    "train": {
        "optimizer": "ADAM",
        "moving_average_decay": 0.9999,          # accepted and ignored: predictions read the raw variables
        "epoch": {"max_nrof_epochs": 2, "size": 250},
        "learning_rate_schedule": {"initial_value": 0.01, "decay_rate": 0.1, "decay_steps": None},
    },
    "embeddings": {"path": "~/datasets/vggface2/test_extracted_160_default/embeddings.npz", "nrof_classes": None,
                   "max_nrof_images": 50, "normalize": False},
}


def load_options(path=None, overrides: dict = None) -> Config:
    """DEFAULTS <- yaml file <- overrides; classifier.path gets a timestamped subdirectory (config.py:247-262 of the
    reference), logfile = classifier.path/log.txt; seeds `random` and NumPy."""
    cfg = dict(DEFAULTS)
    if path is not None:
        import yaml
        with open(Path(path).expanduser()) as f:
            cfg = _merge(cfg, yaml.safe_load(f) or {})
    if overrides:
        cfg = _merge(cfg, overrides)
    c = Config(cfg)
    c.classifier.path = Path(c.classifier.path).expanduser() / datetime.strftime(datetime.now(), "%Y%m%d-%H%M%S")
    c.logdir = c.classifier.path
    c.logfile = c.logdir / "log.txt"
    random.seed(c.seed)
    np.random.seed(c.seed)
    return c


def write_text_log(file, info):
    """ioutils.py:211-218."""
    info_str = 64 * "-" + "\n" + str(info)
    if info_str[-1] != "\n":
        info_str += "\n"
    with Path(file).open(mode="a") as f:
        f.write(info_str)


class ConfusionMatrix:
    """train_classifier.py:17-57.  The per-class-pair prediction counts come from one fn_f2f_pair_counts launch over the
    class-grouped table; the means are summed on the host in float64, in the reference's loop order."""

    def __init__(self, embeddings, classifier):
        nrof_classes = len(embeddings)
        if nrof_classes < 2:
            raise ValueError(f"ConfusionMatrix needs at least 2 classes, got {nrof_classes}")
        sizes = [len(e) for e in embeddings]
        if min(sizes) < 1:
            raise ValueError("ConfusionMatrix: empty class")
        self.counts = pair_counts(embeddings, classifier)
        counts = self.counts.tolist()
        nrof_positive_class_pairs = nrof_classes
        nrof_negative_class_pairs = nrof_classes * (nrof_classes - 1) / 2

        tp = tn = fp = fn = 0
        for i in range(nrof_classes):
            base = i * (i + 1) // 2
            for k in range(i):
                mean = counts[base + k] / (sizes[i] * sizes[k])
                fp += mean
                tn += 1 - mean
            mean = counts[base + i] / (sizes[i] * sizes[i])
            tp += mean
            fn += 1 - mean

        tp /= nrof_positive_class_pairs
        fn /= nrof_positive_class_pairs
        fp /= nrof_negative_class_pairs
        tn /= nrof_negative_class_pairs

        self.classifier = classifier
        self.tp, self.tn, self.fp, self.fn = tp, tn, fp, fn
        self.accuracy = (tp + tn) / (tp + fp + tn + fn)
        self.precision = tp / (tp + fp)
        self.tp_rate = tp / (tp + fn)
        self.tn_rate = tn / (tn + fp)

    def __repr__(self):
        return (f"{self.__class__.__name__}\n" +
                f"{str(self.classifier)}\n" +
                f"accuracy  {self.accuracy}\n" +
                f"precision {self.precision}\n" +
                f"tp rate   {self.tp_rate}\n" +
                f"tn rate   {self.tn_rate}\n")


def pair_counts(embeddings, classifier, table=None, norms=None) -> np.ndarray:
    """int64 [C (C+1) / 2]: slot i (i+1)/2 + k (k <= i) = #(d < threshold) over classes i x k (fn_f2f_pair_counts)."""
    dev = classifier.device
    sizes = [len(e) for e in embeddings]
    if table is None:
        table = as_table(np.concatenate([np.asarray(e, dtype=np.float32) for e in embeddings]), dev)
    if norms is None and classifier.mode == FaceToFaceDistanceClassifier.mode:
        norms = row_norms(table)
    starts = torch.as_tensor(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32), device=dev)
    C = len(sizes)
    out = torch.empty(C * (C + 1) // 2, dtype=torch.int64, device=dev)
    _lib.check(_lib.load().fn_f2f_pair_counts(ptr(table), ptr(norms), ptr(starts), C, table.shape[1], classifier.mode,
                                              ptr(classifier.params), ptr(out), stream(dev)), "f2f_pair_counts")
    return out.cpu().numpy()


def learning_rate(schedule, epoch_size, global_step: int) -> float:
    """train_classifier.py:112-125: initial_value * decay_rate ^ floor(global_step / decay_steps), in float64."""
    decay_steps = schedule.decay_steps if schedule.decay_steps else epoch_size
    return float(schedule.initial_value) * float(schedule.decay_rate) ** math.floor(global_step / float(decay_steps))


def train_classifier(options, device="cuda", log=print):
    check_optimizer(options.train.optimizer)
    options.logdir.mkdir(parents=True, exist_ok=True)
    embeddings = Embeddings(options.embeddings)
    write_text_log(options.logfile, embeddings)
    log(embeddings)

    embarray = embeddings.data(normalize=options.embeddings.normalize)
    batches = equal_batches_input_pipeline(embarray, options)

    if options.embeddings.normalize:
        model = FaceToFaceNormalizedEmbeddingsClassifier(device=device)
    else:
        model = FaceToFaceDistanceClassifier(device=device)

    schedule, epoch = options.train.learning_rate_schedule, options.train.epoch
    trainer = ClassifierTrainer(model, embarray, options.nrof_classes_per_batch, options.nrof_examples_per_class,
                                learning_rate=learning_rate(schedule, epoch.size, 0), optimizer=options.train.optimizer)
    trainer.capture()                     # side-effect free; batches are drawn after it, as an eager run would draw them
    log("start training")
    global_step, lr = 0, None
    for ep in range(epoch.max_nrof_epochs):
        for _ in range(epoch.size):
            step_lr = learning_rate(schedule, epoch.size, global_step)
            if step_lr != lr:
                trainer.set_learning_rate(step_lr)
                lr = step_lr
            trainer.step(next(batches))
            global_step += 1
        info = f"epoch [{ep + 1}/{epoch.max_nrof_epochs}], learning rate {lr}, loss {trainer.loss_value()}"
        log(info)
        conf_mat = ConfusionMatrix(embarray, model)
        log(conf_mat)
        write_text_log(options.logfile, info)
        write_text_log(options.logfile, conf_mat)

    model.save(options.classifier.path / "classifier.npz")
    log(f"Model has been saved to the directory: {options.classifier.path}")
    return model, trainer


@click.command()
@click.option("--config", default=None, type=Path, help="Path to yaml config file with used options for the application.")
def main(**options):
    train_classifier(load_options(options["config"]))


if __name__ == "__main__":
    main()
