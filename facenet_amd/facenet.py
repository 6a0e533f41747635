"""Helpers on the hot path, same names and behaviour as facenet/facenet.py:
``inputs`` (:35-36), ``ImageProcessing`` (:57-86), ``evaluate_embeddings`` (:184-201),
``LearningRateScheduler`` (:381-400), and the pair-classifier data path ``split_embeddings``, ``Embeddings``
(:220-296) and ``equal_batches_input_pipeline`` (:89-123)."""
from __future__ import annotations

import numpy as np
import torch


def inputs(config):
    """facenet.py:35-36 returns ``tf.keras.Input([size, size, 3])``; here the symbolic shape itself."""
    return (config.size, config.size, 3)


class ImageProcessing:
    """Input normalisation layer (facenet.py:57-86).  It carries the configuration; the arithmetic runs
    in fn_image_normalize as the first launch of every plan (fused there with the channel padding)."""

    def __init__(self, config):
        self.input_node_name = "input"
        self.config = config
        self.image_size = (config.size, config.size)
        self.eps = 1e-3
        if config.normalization not in (0, 1):
            raise ValueError("Invalid image normalization algorithm")   # facenet.py:82


def evaluate_embeddings(model, dset):
    """facenet.py:184-201: run ``model(images)`` over (images, labels) batches and concatenate."""
    embeddings_, labels_ = [], []
    for images, labels in dset:
        emb = model(images)
        embeddings_.append(emb.detach().cpu().numpy() if torch.is_tensor(emb) else np.asarray(emb))
        labels_.append(np.asarray(labels))
    return np.concatenate(embeddings_), np.concatenate(labels_)


class LearningRateScheduler:
    """facenet.py:381-400 (0-based epoch; constant when ``config.value`` is set)."""

    def __init__(self, config):
        self.config = config
        self.default_value = self.config.value if self.config.value else None

    def __call__(self, epoch):
        if self.default_value is not None:
            return self.default_value
        learning_rate = self.config.schedule[-1][1]
        for (epoch_, learning_rate) in self.config.schedule:
            if epoch < epoch_:
                break
        return learning_rate


# ------------------------------------------------------------------------------------------------------------------
# Embeddings file and the equal-batches sampler of the pair classifier (facenet.py:89-123, :220-296)
# ------------------------------------------------------------------------------------------------------------------
def split_embeddings(embeddings, labels):
    """facenet.py:220-225: one array per distinct label, labels in ascending order."""
    labels = np.asarray(labels)
    return [embeddings[label == labels] for label in np.unique(labels)]


class Embeddings:
    """facenet.py:228-296.  ``config.path`` is an ``.npz`` with ``embeddings`` [N, E] and ``labels`` [N] (as written by
    facenet_amd.apps.embeddings); ``nrof_classes`` and ``max_nrof_images`` subsample with ``random.sample`` as the reference
    does."""

    def __init__(self, config):
        import random
        from pathlib import Path

        self.config = config
        self.file = Path(config.path).expanduser()
        if self.file.suffix == ".h5":
            raise ValueError(f"{self.file}: .h5 embeddings files need h5py, which this project does not use; "
                             "write an .npz with 'embeddings' and 'labels' (facenet_amd.apps.embeddings)")
        with np.load(self.file) as f:
            embeddings = np.asarray(f["embeddings"], dtype=np.float32)
            labels = np.asarray(f["labels"])
        self.embeddings = split_embeddings(embeddings, labels)

        if self.config.nrof_classes:
            if self.nrof_classes > self.config.nrof_classes:
                labels = random.sample(list(range(self.nrof_classes)), self.config.nrof_classes)
                self.embeddings = [self.embeddings[label] for label in labels]

        if self.config.max_nrof_images:
            for idx, emb in enumerate(self.embeddings):
                nrof_images = emb.shape[0]
                if nrof_images > self.config.max_nrof_images:
                    labels = random.sample(list(range(nrof_images)), self.config.max_nrof_images)
                    self.embeddings[idx] = self.embeddings[idx][labels, :]

    def __repr__(self):
        data = [len(e) for e in self.embeddings]
        norm = np.linalg.norm(np.concatenate(self.embeddings, axis=0), axis=1)
        return (f"{self.__class__.__name__}\n" +
                f"Input file {self.file}\n" +
                f"Number of classes {self.nrof_classes} \n" +
                f"Number of images {self.nrof_images}\n" +
                f"Minimal number of images in class {min(data)}\n" +
                f"Maximal number of images in class {max(data)}\n" +
                "\n" +
                f"Minimal embedding {np.min(norm)}\n" +
                f"Maximal embedding {np.max(norm)}\n" +
                f"Mean embedding {np.mean(norm)}\n")

    @property
    def nrof_classes(self):
        return len(self.embeddings)

    @property
    def nrof_images(self):
        return sum(len(e) for e in self.embeddings)

    @property
    def length(self):
        return self.embeddings[0].shape[1]

    def data(self, normalize=False):
        """The per-class arrays; with ``normalize`` every row divided by its L2 norm.  Unlike the reference (which divides
        its own arrays in place) the stored embeddings are left as they are and normalised copies are returned."""
        if not normalize:
            return self.embeddings
        return [(e / np.linalg.norm(e, axis=1, keepdims=True)).astype(np.float32) for e in self.embeddings]


def equal_batches_input_pipeline(embeddings, config):
    """facenet.py:89-123.  ``embeddings``: per-class arrays.  Yields int32 arrays of P K row indices into their concatenation
    (the class-grouped table of ClassifierTrainer), class by class: ``random.sample`` of P classes, then of K rows of each, in
    the reference generator's order, so the same ``random`` state picks the same rows.  P and K are written back into
    ``config`` as the reference does.  Raises ValueError for K < 2, P > the number of classes or a class with fewer than K rows
    (every class can be sampled), before anything runs."""
    import random

    if not embeddings:
        raise ValueError("equal_batches_input_pipeline: no classes")
    if not config.nrof_classes_per_batch:
        config.nrof_classes_per_batch = len(embeddings)
    if not config.nrof_examples_per_class:
        config.nrof_examples_per_class = round(0.1 * sum([len(embs) for embs in embeddings]) / len(embeddings))
        config.nrof_examples_per_class = max(config.nrof_examples_per_class, 1)
    P, K = int(config.nrof_classes_per_batch), int(config.nrof_examples_per_class)
    if K < 2:
        raise ValueError(f"nrof_examples_per_class must be at least 2 (a batch needs positive pairs), got {K}")
    if P > len(embeddings):
        raise ValueError(f"nrof_classes_per_batch {P} exceeds the {len(embeddings)} classes")
    sizes = [len(e) for e in embeddings]
    small = [c for c, n in enumerate(sizes) if n < K]
    if small:
        raise ValueError(f"{len(small)} classes (first: class {small[0]} with {sizes[small[0]]} rows) have fewer than "
                         f"nrof_examples_per_class = {K} rows")

    print("building equal batches input pipeline.")
    print("number of classes per batch ", P)
    print("number of examples per class", K)
    starts = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)

    def generator():
        while True:
            rows = []
            for c in random.sample(range(len(embeddings)), P):
                rows += [starts[c] + i for i in random.sample(range(sizes[c]), K)]
            yield np.asarray(rows, dtype=np.int32)

    return generator()
