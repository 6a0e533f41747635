# coding:utf-8
"""Validation inside training: facenet/callbacks.py:12-28 of the reference (``ValidateCallback``), wired into the training
apps the way apps/train_softmax.py:41-45,85-88 wires it into ``fit``.

Every ``every_n_epochs`` epochs and after the last one the held-out data set is embedded with the model being trained, in
inference mode, and a ``FaceToFaceValidation`` report is logged and appended to ``<model.path>/report.txt``."""
from __future__ import annotations

import contextlib
import time
from pathlib import Path

import numpy as np
import torch

from ._call import host_array

# A validation set whose decoded uint8 images (nrof_images * size * size * 3 bytes) fit in this many bytes stays on the device
# after the first pass; a larger one is streamed from disk on every pass.  The reference's 26 489-image set is 2.0 GB.
RESIDENT_BYTES = 4 << 30


def validation_due(epoch: int, every_n_epochs: int, max_nrof_epochs) -> bool:
    """callbacks.py:21-24 for the 0-based ``epoch`` that just ended."""
    epoch1 = epoch + 1
    return epoch1 % every_n_epochs == 0 or epoch1 == max_nrof_epochs


def shard(nrof_batches: int, rank: int, world: int):
    """The batch indices rank ``rank`` of ``world`` embeds: rank, rank + world, ..."""
    return list(range(rank, nrof_batches, world))


def interleave(per_rank):
    """per_rank[r] = the arrays rank r produced for its batches ``shard(n, r, world)``, in its own order -> the arrays of all
    batches in data-set order (batch j is entry j // world of rank j % world)."""
    world = len(per_rank)
    total = sum(len(p) for p in per_rank)
    for r, p in enumerate(per_rank):
        if len(p) != len(shard(total, r, world)):
            raise ValueError("rank {} holds {} batches, expected {} of {}".format(r, len(p), len(shard(total, r, world)), total))
    return [per_rank[j % world][j // world] for j in range(total)]


class TrainerModel:
    """The model a Trainer is training as the callable ``ValidateCallback`` wants: uint8 [N,S,S,3] -> unit-norm embeddings,
    from the raw weights or (``averaged``) from the moving average.  ``validation_pass()`` brackets one pass over the data
    set, so the average is swapped into the weights and refolded once per pass, not once per batch."""

    def __init__(self, trainer, averaged: bool = False, path=None):
        if averaged and trainer.shadow is None:
            raise ValueError("validate.averaged needs train.moving_average_decay: this trainer keeps no moving average")
        self.trainer, self.averaged, self.path = trainer, bool(averaged), path

    def validation_pass(self):
        return self.trainer.averaged_weights() if self.averaged else contextlib.nullcontext()

    def __call__(self, images):
        return self.trainer.evaluate(images, averaged=self.averaged)


class ValidateCallback:
    """``ValidateCallback(model, dataset, every_n_epochs, max_nrof_epochs, config)`` of callbacks.py:12-28.

    ``model``: callable from uint8 images to unit-norm embeddings (``None``: the training app attaches its trainer);
    ``dataset``: an iterable of (images, labels) that can be walked repeatedly; ``config.validate``: metric, nrof_folds,
    far_target, and far_targets (optional: the exact VerificationCurve at these rates follows the report and is set on it as
    ``report.curve``; fpir_targets / fpir_rank, optional: the open-set IdentificationCurve follows likewise as
    ``report.identification``; without a key the report object is left as the statistic made it).
    ``history`` collects (epoch, FaceToFaceValidation.dict, seconds embedding, seconds statistics).

    Data parallel: every rank embeds the batches ``rank::world``, the embeddings are all-gathered in data-set order, rank 0
    computes, logs and writes the report; ``on_epoch_end`` is collective."""

    def __init__(self, model, dataset, every_n_epochs, max_nrof_epochs, config, averaged: bool = False, log=print, rank: int = 0,
                 world: int = 1, process_group=None, statistic=None, device=None, resident_bytes: int = RESIDENT_BYTES):
        if every_n_epochs is None or int(every_n_epochs) < 1:
            raise ValueError("every_n_epochs must be at least 1, got {}".format(every_n_epochs))
        self._model = model
        self.dataset = dataset
        self.config = config
        self.every_n_epochs = int(every_n_epochs)
        self.max_nrof_epochs = max_nrof_epochs
        self.averaged = bool(averaged)
        self.log, self.rank, self.world, self.process_group = log, rank, world, process_group
        self.statistic = statistic
        self.device, self.resident_bytes = device, resident_bytes
        self.history = []
        self.embeddings = self.labels = None          # of the last pass (rank 0)
        self._resident = None                           # this rank's batches on the device, once they have been decoded

    @property
    def model(self):
        return self._model

    def attach(self, trainer, path=None, rank: int = 0, world: int = 1, process_group=None):
        """Bind the callback to the trainer of a training app."""
        self._model = TrainerModel(trainer, averaged=self.averaged, path=path)
        self.rank, self.world, self.process_group = rank, world, process_group
        if self.device is None:
            self.device = trainer.net.device
        return self

    # ---- one pass over the data set ----------------------------------------------------------------------------------------
    def _batches(self):
        """This rank's (images, labels) batches; kept on the device after the first pass when they fit in resident_bytes."""
        if self._resident is not None:
            yield from self._resident
            return
        kept, nbytes = [], 0
        for j, (images, labels) in enumerate(self.dataset):
            if j % self.world != self.rank:
                continue
            labels = host_array(labels)
            if kept is not None:
                x = torch.as_tensor(images)
                x = x.to(self.device, copy=True) if self.device is not None else x.clone()    # a copy: pipelines may reuse buffers
                nbytes += x.numel() * x.element_size() * self.world      # the whole set's size decides, not the shard's
                if nbytes > self.resident_bytes:
                    kept = None                                          # too large: every pass streams
                else:
                    kept.append((x, labels))
                    images = x
            yield images, labels
        if kept is not None:
            self._resident = kept

    def embed(self):
        """(embeddings [n, E], labels [n]) of the whole data set in data-set order on every rank.  Collective."""
        model = self._model
        emb, lab = [], []
        with getattr(model, "validation_pass", contextlib.nullcontext)():
            for images, labels in self._batches():
                e = model(images)
                emb.append(e.detach().cpu().numpy() if torch.is_tensor(e) else np.asarray(e))
                lab.append(labels)
        if self.world > 1:
            import torch.distributed as dist
            gathered = [None] * self.world
            dist.all_gather_object(gathered, (emb, lab), group=self.process_group)
            emb, lab = interleave([g[0] for g in gathered]), interleave([g[1] for g in gathered])
        return np.concatenate(emb), np.concatenate(lab)

    def validate(self, epoch1: int):
        if self._model is None:
            raise RuntimeError("ValidateCallback has no model: pass one or attach() a trainer")
        if self.rank == 0:
            self.log(f"perform validation for epoch {epoch1}")
        t0 = time.perf_counter()
        embeddings, labels = self.embed()
        t1 = time.perf_counter()
        if self.rank != 0:
            return None
        statistic = self.statistic
        if statistic is None:
            from .statistics import FaceToFaceValidation as statistic
        report = statistic(embeddings, labels, self.config.validate)
        from .statistics import verification_curve
        curve = verification_curve(embeddings, labels, self.config.validate)        # None unless validate.far_targets is set
        if curve is not None:
            report.curve = curve
        from .statistics import identification_curve
        identification = identification_curve(embeddings, labels, self.config.validate)      # None unless validate.fpir_targets is set
        if identification is not None:
            report.identification = identification
        t2 = time.perf_counter()
        self.embeddings, self.labels = embeddings, labels
        self.history.append((epoch1, report.dict, t1 - t0, t2 - t1))
        self.log(str(report))
        if curve is not None:
            self.log(str(curve))
        if identification is not None:
            self.log(str(identification))
        self.log(f"validation: embedding {t1 - t0:.3f} s, statistics {t2 - t1:.3f} s")
        path = getattr(self._model, "path", None)
        if path:
            path = Path(path).expanduser()
            path.mkdir(parents=True, exist_ok=True)
            report.write_report(path / "report.txt")
            if curve is not None:
                from .apps.train_classifier import write_text_log
                write_text_log(path / "report.txt", curve)
            if identification is not None:
                from .apps.train_classifier import write_text_log
                write_text_log(path / "report.txt", identification)
        return report

    def on_epoch_end(self, epoch, logs=None):
        if validation_due(epoch, self.every_n_epochs, self.max_nrof_epochs):
            return self.validate(epoch + 1)
        return None


def from_config(cfg, log=print, rank: int = 0, **kw):
    """The callback ``cfg.validate`` describes (train_softmax.yaml:94-117), or None when ``validate.dataset.path`` is unset.
    The training app attaches its trainer.  Every rank draws the same images (``max_nrof_images`` samples with NumPy's global
    generator, seeded here with cfg.seed and restored, so the training pipeline's draws are what they are without validation)."""
    if not cfg.validate.dataset.path:
        return None
    from . import dataset
    state = np.random.get_state()
    np.random.seed(cfg.seed)
    try:
        dbase = dataset.Database(cfg.validate.dataset)
    finally:
        np.random.set_state(state)
    if rank == 0:
        log(dbase)
    batches = dbase.tf_dataset_api(loader=dataset.ImageLoader(config=cfg.image), batch_size=cfg.batch_size, repeat=False,
                                   buffer_size=None, **kw)
    return ValidateCallback(None, batches, cfg.validate.every_n_epochs, cfg.train.epoch.nrof_epochs, cfg.validate,
                            averaged=bool(cfg.validate.averaged), log=log, rank=rank)
