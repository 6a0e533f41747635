# coding:utf-8
"""Softmax-classifier training entry point, same shape as the reference's apps/train_softmax.py:21-112:
``python -m facenet_amd.apps.train_softmax --config x.yaml``.

model = InceptionResnetV1; network = Sequential([model, Dense(nrof_classes)]) (:55-66); loss =
SparseCategoricalCrossentropy(from_logits=True) (:91); Adam(epsilon=0.1) (:92), or the Keras optimizer train.optimizer names
(DESIGN.md section 15); LR set per epoch by
LearningRateScheduler (:80-83); ``train.epoch.size`` steps per epoch (:95-104).

Batches come from ``batches`` (an iterable of (uint8 images [N,160,160,3], int labels [N])); ``main`` builds them from
``cfg.dataset.path`` with facenet_amd.dataset (Database + tf_dataset_api, :28-47 of the reference app) or, when no data
set is configured, from a seeded synthetic generator."""
from __future__ import annotations

import time
from pathlib import Path

import click
import numpy as np
import torch

from facenet_amd import config as config_mod
from facenet_amd.engine_v2 import build_network
from facenet_amd.facenet import LearningRateScheduler
from facenet_amd.train import Trainer, moving_average_decay, optimizer_name


def synthetic_batches(batch_size, nrof_classes, size, seed):
    g = torch.Generator().manual_seed(seed)
    while True:
        yield (torch.randint(0, 256, (batch_size, size, size, 3), dtype=torch.uint8, generator=g),
               torch.randint(0, nrof_classes, (batch_size,), generator=g))


def init_distributed():
    """One process per GPU under ``python -m torch.distributed.run``: (rank, world, process group, device).  Without the
    launcher's environment: a single replica.  ``MirroredStrategy()`` of apps/train_softmax_tf2_gpus.py:49 becomes RCCL
    (backend "nccl") over xGMI; FACENET_DIST_BACKEND=gloo rehearses the same path on one device."""
    import os
    world, rank, local = (int(os.environ.get(k, d)) for k, d in (("WORLD_SIZE", "1"), ("RANK", "0"), ("LOCAL_RANK", "0")))
    if world == 1:
        return 0, 1, None, "cuda"
    import torch.distributed as dist
    backend = os.environ.get("FACENET_DIST_BACKEND", "nccl")
    dev_index = local if backend == "nccl" else local % max(1, torch.cuda.device_count())
    torch.cuda.set_device(dev_index)
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    if not dist.is_initialized():
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", dev_index))
        else:
            dist.init_process_group(backend)
    return rank, world, dist.group.WORLD, f"cuda:{dev_index}"


def train_softmax(cfg, nrof_classes: int, batches=None, embedding_size: int = 512, device: str = "cuda", use_graph: bool = True,
                  world_size: int = 1, process_group=None, rank: int = 0, log=print, validation=None):
    """``cfg.batch_size`` is the GLOBAL batch: MirroredStrategy splits it across the replicas
    (apps/train_softmax_tf2_gpus.py:49-108), so every rank trains ``cfg.batch_size // world_size`` images per step with
    per-replica BatchNorm, gradients are averaged over the global batch, and ``batches`` must yield this rank's shard.
    ``validation``: a facenet_amd.callbacks.ValidateCallback (:41-45,85-88), called after every epoch on every rank."""
    if cfg.batch_size % world_size:
        raise ValueError(f"batch_size {cfg.batch_size} is not divisible by the {world_size} replicas")
    local_batch = cfg.batch_size // world_size
    optimizer = optimizer_name(cfg)                               # train.optimizer (train_softmax.yaml:25-26): checked before any GPU work
    # model.module picks the family (Inception-ResNet-v1 by default, v2 for facenet[_amd].models.inception_resnet_v2)
    net = build_network(cfg.model, embedding_size, image_size=cfg.image.size, normalization=cfg.image.normalization,
                        nrof_classes=nrof_classes, device=device, seed=cfg.seed)
    scheduler = LearningRateScheduler(cfg.train.learning_rate)
    # loss.center_* / prelogits_norm_* (train_softmax.yaml:73-78): center loss and prelogits-norm loss on the embedding;
    # train.moving_average_decay (:28): the moving average of the weights; loss.margin_*: the large-margin cosine softmax head
    trainer = Trainer(net, batch=local_batch, loss="softmax", lr=scheduler(0), world_size=world_size, process_group=process_group,
                      moving_average_decay=moving_average_decay(cfg), optimizer=optimizer,
                      **{k: _loss_key(cfg, k) for k in ("center_factor", "center_alfa", "prelogits_norm_factor", "prelogits_norm_p",
                                                       "margin_scale", "margin_arc", "margin_cos")})
    if rank == 0 and trainer.margin:                             # once; a plain softmax run logs exactly what it always did
        log(f"margin softmax: scale {trainer.margin_scale:g}  arc {trainer.margin_arc:g}  cos {trainer.margin_cos:g}")
    if rank == 0 and optimizer != "ADAM":                        # once; an Adam run logs exactly what it always did
        log(f"optimizer: {optimizer}")
    if validation is not None and validation.model is None:      # ValidateCallback(model=network, ...) of :85-88
        validation.attach(trainer, path=cfg.model.path if cfg.model.path else None, rank=rank, world=world_size, process_group=process_group)
    first_epoch = 0
    if cfg.model.checkpoint:                                      # network.load_weights(checkpoint) before fit (:68-71)
        ckpt = Path(cfg.model.checkpoint).expanduser()
        ckpt = ckpt / f"{ckpt.stem}.npz" if ckpt.is_dir() else ckpt
        log(f"Restore checkpoint {ckpt}")
        first_epoch = trainer.load_checkpoint(ckpt)
    if batches is None:
        batches = synthetic_batches(local_batch, nrof_classes, cfg.image.size, cfg.seed + rank)    # a different shard per rank
    batches = iter(batches)
    if use_graph:
        x, y = next(batches)
        trainer.set_images(x, y)
        trainer.capture()                                         # side-effect free: no uncounted step, Adam's t untouched
        batches = _chain_first((x, y), batches)                   # the batch used for the capture is trained on as batch 1
    for epoch in range(first_epoch, cfg.train.epoch.nrof_epochs):
        trainer.set_learning_rate(scheduler(epoch))              # Keras LearningRateScheduler callback: 0-based epoch
        t0 = time.perf_counter()
        for _ in range(cfg.train.epoch.size):
            x, y = next(batches)
            trainer.set_images(x, y)
            trainer.step()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if rank == 0:
            reg = ""
            if trainer.regularized:                               # the reference's logged names (models/*/logs/report.h5)
                t = trainer.loss_terms()
                reg = "".join(f"  {k} {t[k]:.4f}" for k in ("center_loss", "prelogits_norm", "loss") if t[k] is not None)
            log(f"epoch {epoch + 1}/{cfg.train.epoch.nrof_epochs}  xent {trainer.loss_value():.4f}{reg}  lr {scheduler(epoch)}  "
                f"{cfg.batch_size * cfg.train.epoch.size / dt:.1f} img/s")
        if cfg.model.path:                                        # ModelCheckpoint(save_weights_only=True) each epoch (:74-78)
            path = Path(cfg.model.path).expanduser()
            if rank == 0:
                path.mkdir(parents=True, exist_ok=True)
            # Keras variable names and order + optimizer slots, iteration count and epoch; moving statistics averaged over replicas
            trainer.save_checkpoint(path / f"{path.stem}.npz", epoch=epoch + 1)
            if trainer.shadow is not None:                        # the averaged model, loadable by FaceNet(config.path=...)
                if rank == 0:
                    (path / "averaged").mkdir(exist_ok=True)
                trainer.save_averaged_weights(path / "averaged" / f"{path.stem}.npz")
        if validation is not None:                                # after ModelCheckpoint, as in the reference's callback list
            validation.on_epoch_end(epoch)
    return net, trainer


def dataset_batches(cfg, rank: int = 0, world: int = 1, log=print, **kw):
    """apps/train_softmax.py:28-47: (Database of cfg.dataset.path, this rank's endless shuffled batch pipeline).  The image.random_*
    keys (train_softmax.yaml:85-91) augment the batches, drawn from a generator seeded by seed + rank; rank 0 logs them once.
    dataset.resident (with resident_cache, resident_bytes): the same batches from a decoded copy of the set in device memory."""
    from facenet_amd import dataset
    loader = dataset.ImageLoader(config=cfg.image)
    train_dbase = dataset.Database(cfg.dataset)
    augment = dataset.Augmentation.from_config(cfg.image, cfg.seed + rank)
    if augment is not None and rank == 0:
        log(f"augmentation: {augment}")
    store = None
    if cfg.dataset.resident:                                      # the decoded set in device memory; every
        from facenet_amd import resident                          # rank holds all of it, since every rank walks all of it
        store = resident.from_config(cfg.dataset, train_dbase, device=kw.get("device", "cuda"), rank=rank, log=log)
    np.random.seed(cfg.seed + rank)                               # every replica walks its own permutation of the data set
    kw.setdefault("processes", True)
    batches = train_dbase.tf_dataset_api(loader=loader, batch_size=cfg.batch_size // world, repeat=True, buffer_size=10,
                                         augment=augment, resident=store, **kw)
    return train_dbase, batches


def _loss_key(cfg, key):
    """cfg.loss.<key>, or the reference default when the settings tree lacks it (a Config not built by load_config)."""
    return cfg.loss.as_dict[key] if cfg.loss.exists(key) else config_mod.DEFAULTS["loss"][key]


def _chain_first(first, rest):
    yield first
    yield from rest


@click.command()
@click.option("--config", default=None, type=Path, help="Path to yaml config file with used options of the application.")
@click.option("--nrof-classes", default=10575, type=int, help="Number of identities (synthetic data when no dataset is wired in).")
def main(**options):
    cfg = config_mod.load_config(options["config"])
    rank, world, pg, device = init_distributed()                  # python -m torch.distributed.run --nproc-per-node N -m facenet_amd.apps.train_softmax
    kw = dict(device=device, world_size=world, process_group=pg, rank=rank)
    from facenet_amd import callbacks
    kw["validation"] = callbacks.from_config(cfg, rank=rank)     # None unless validate.dataset.path is set
    if cfg.dataset.path:
        train_dbase, batches = dataset_batches(cfg, rank, world)
        train_softmax(cfg, train_dbase.nrof_classes, batches, **kw)
    else:
        train_softmax(cfg, options["nrof_classes"], **kw)


if __name__ == "__main__":
    main()
