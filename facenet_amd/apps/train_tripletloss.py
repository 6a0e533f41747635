# coding:utf-8
"""Triplet-loss training entry point (the north-star path; the reference only mentions it at README.md:18 -- build-defined,
SURVEY.md A13): ``python -m facenet_amd.apps.train_tripletloss --config x.yaml``.

Per step: embed a P x K pool with the inference path -> [PK,PK] squared distances -> online selection (alpha) ->
train on the selected (a,p,n) rows: forward(training=True) -> l2_normalize -> triplet loss -> backward -> the Keras optimizer
train.optimizer names (Adam by default).
Pools come from ``pools`` (an iterable of (uint8 images [P*K,160,160,3])) with labels repeat(arange(P), K) or, by
default, from a seeded synthetic generator.

``loss.triplet_strategy: batch_hard | batch_all`` (with ``loss.soft_margin``) trains on the whole P x K batch instead and mines
inside it (arXiv 1703.07737 sec. 2): no pool forward, no selection, no gather; per step set_images(images,
labels) -> step.  ``pools`` may then yield ``images`` or ``(images, labels)``.  Absent or ``mined``: the behaviour above.

``loss.memory_size: M`` (with ``loss.memory_start``: the steps to let pass before rows are stored) adds a cross-batch memory of the last M
embedded rows to ``batch_hard`` (Wang et al., CVPR 2020).  Its labels must mean the same identity in every
step, so ``pools`` must then yield ``(images, labels)`` with dataset-wide identity ids."""
from __future__ import annotations

import time
from pathlib import Path

import click
import numpy as np
import torch

from facenet_amd import config as config_mod
from facenet_amd.engine_v2 import build_network
from facenet_amd.facenet import LearningRateScheduler
from facenet_amd.heads import TRIPLET_STRATEGIES
from facenet_amd.train import GraphRunner, Trainer, TripletMiner, moving_average_decay, optimizer_name
from facenet_amd.schedule import make_events


def triplet_settings(cfg):
    """(loss.triplet_strategy, loss.soft_margin): absent keys mean the mined step and the hinge."""
    strategy = cfg.loss.triplet_strategy if cfg.loss.triplet_strategy else "mined"
    if strategy not in TRIPLET_STRATEGIES:
        raise ValueError(f"loss.triplet_strategy must be one of {', '.join(TRIPLET_STRATEGIES)}, got {strategy!r}")
    return strategy, bool(cfg.loss.soft_margin)


def memory_settings(cfg):
    """(loss.memory_size, loss.memory_start): absent keys mean no cross-batch memory.  Whole numbers only; their ranges are the
    Trainer's to refuse (heads.check_loss_arguments)."""
    out = []
    for key in ("memory_size", "memory_start"):
        v = getattr(cfg.loss, key)
        v = 0 if v is None or isinstance(v, config_mod.Config) and not v else v      # (an absent key reads as an empty Config)
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 0:
            raise ValueError(f"loss.{key} must be a non-negative integer, got {v!r}")
        out.append(int(v))
    return tuple(out)


def end_of_epoch(cfg, trainer, validation, epoch):
    if trainer.shadow is not None and cfg.model.path:            # the averaged model, loadable by FaceNet(config.path=...)
        path = Path(cfg.model.path).expanduser()
        if trainer.rank == 0:
            (path / "averaged").mkdir(parents=True, exist_ok=True)
        trainer.save_averaged_weights(path / "averaged" / f"{path.stem}.npz")
    if validation is not None:
        validation.on_epoch_end(epoch)


def train_batch_triplet(cfg, net, strategy, soft, alpha, optimizer, people_per_batch, images_per_person, pools, use_graph, world_size,
                        process_group, log, validation, memory_size=0, memory_start=0):
    """The batch-mined run: the trainer's batch is the whole P x K batch and every embedded image receives a gradient."""
    n = people_per_batch * images_per_person
    scheduler = LearningRateScheduler(cfg.train.learning_rate)
    trainer = Trainer(net, batch=n, loss="triplet", alpha=alpha, lr=scheduler(0), world_size=world_size, process_group=process_group,
                      moving_average_decay=moving_average_decay(cfg), optimizer=optimizer, triplet_strategy=strategy, soft_margin=soft,
                      **(dict(memory_size=memory_size, memory_start=memory_start) if memory_size else {}))
    if trainer.rank == 0:
        log(f"triplet strategy: {strategy}" + (", soft margin" if soft else "") + (f", optimizer: {optimizer}" if optimizer != "ADAM" else "")
            + (f", cross-batch memory: {memory_size} rows from step {memory_start}" if memory_size else ""))
    if validation is not None and validation.model is None:
        validation.attach(trainer, path=cfg.model.path if cfg.model.path else None, rank=trainer.rank, world=world_size,
                          process_group=process_group)
    default_labels = np.repeat(np.arange(people_per_batch), images_per_person)
    if pools is None:
        g = torch.Generator().manual_seed(cfg.seed)
        pools = (torch.randint(0, 256, (n, cfg.image.size, cfg.image.size, 3), dtype=torch.uint8, generator=g) for _ in iter(int, 1))
    pools = iter(pools)

    def feed():
        item = next(pools)
        if memory_size and not isinstance(item, (tuple, list)):
            # repeat(arange(P), K) restarts at 0 in every batch: in the memory, rows of different people would share an id
            raise ValueError("with loss.memory_size the pools must yield (images, labels) with dataset-wide identity ids")
        images, labels = item if isinstance(item, (tuple, list)) else (item, default_labels)
        trainer.set_images(images, labels)

    if use_graph:
        trainer.set_images(torch.zeros_like(trainer.plan.images), default_labels)      # the warm-up step of capture() needs a live batch
        trainer.capture()                                         # side-effect free (state restored after its warm-up step)
    for epoch in range(cfg.train.epoch.nrof_epochs):
        trainer.set_learning_rate(scheduler(epoch))
        t0 = time.perf_counter()
        for _ in range(cfg.train.epoch.size):
            feed()
            trainer.step()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        stats = trainer.triplet_stats()
        log(f"epoch {epoch + 1}/{cfg.train.epoch.nrof_epochs}  triplet loss {trainer.loss_value():.4f}  "
            f"active {stats['active_fraction']:.3f} ({stats['active']}/{stats['terms']})  "
            + (f"memory negatives {stats['memory_negatives'] / max(stats['anchors'], 1):.3f} ({stats['memory_valid']} rows)  " if memory_size else "") +
            f"{n * cfg.train.epoch.size * world_size / dt:.1f} img/s")
        end_of_epoch(cfg, trainer, validation, epoch)
    return net, trainer


def train_tripletloss(cfg, people_per_batch: int = 45, images_per_person: int = 4, nrof_triplets: int = 30, embedding_size: int = 128,
                      pools=None, device: str = "cuda", use_graph: bool = True, world_size: int = 1, process_group=None, log=print,
                      validation=None):
    """``validation``: a facenet_amd.callbacks.ValidateCallback, called after every epoch on every rank."""
    alpha = cfg.loss.alpha if cfg.loss.alpha else 0.2
    optimizer = optimizer_name(cfg)                               # train.optimizer: checked before any GPU work
    # model.module picks the family (Inception-ResNet-v1 by default, v2 for facenet[_amd].models.inception_resnet_v2)
    net = build_network(cfg.model, embedding_size, image_size=cfg.image.size, normalization=cfg.image.normalization,
                        device=device, seed=cfg.seed)
    strategy, soft = triplet_settings(cfg)
    memory_size, memory_start = memory_settings(cfg)
    if memory_size and strategy != "batch_hard":
        raise ValueError("loss.memory_size needs loss.triplet_strategy batch_hard")
    if strategy != "mined":
        return train_batch_triplet(cfg, net, strategy, soft, alpha, optimizer, people_per_batch, images_per_person, pools, use_graph,
                                   world_size, process_group, log, validation, memory_size, memory_start)
    if soft:
        raise ValueError("loss.soft_margin needs loss.triplet_strategy batch_hard or batch_all")
    scheduler = LearningRateScheduler(cfg.train.learning_rate)
    trainer = Trainer(net, batch=3 * nrof_triplets, loss="triplet", alpha=alpha, lr=scheduler(0), world_size=world_size,
                      process_group=process_group, moving_average_decay=moving_average_decay(cfg), optimizer=optimizer)
    if trainer.rank == 0 and optimizer != "ADAM":                # once; an Adam run logs exactly what it always did
        log(f"optimizer: {optimizer}")
    if validation is not None and validation.model is None:
        validation.attach(trainer, path=cfg.model.path if cfg.model.path else None, rank=trainer.rank, world=world_size,
                          process_group=process_group)
    n = people_per_batch * images_per_person
    miner = TripletMiner(net, n, np.repeat(np.arange(people_per_batch), images_per_person), nrof_triplets, alpha=alpha, seed=cfg.seed)
    miner.build(trainer.plan.images)
    if pools is None:
        g = torch.Generator().manual_seed(cfg.seed)
        pools = (torch.randint(0, 256, (n, cfg.image.size, cfg.image.size, 3), dtype=torch.uint8, generator=g) for _ in iter(int, 1))
    pools = iter(pools)
    mine_graph = None
    if use_graph:
        miner.plan.images.copy_(next(pools))
        miner.run()
        ev = make_events(miner.sched)
        mine_graph = GraphRunner(net.device).capture(lambda: miner.run(ev))
        trainer.capture()                                         # side-effect free (state restored after its warm-up step)
    for epoch in range(cfg.train.epoch.nrof_epochs):
        trainer.set_learning_rate(scheduler(epoch))
        t0 = time.perf_counter()
        for _ in range(cfg.train.epoch.size):
            miner.plan.images.copy_(next(pools))
            mine_graph.replay() if mine_graph is not None else miner.run()
            trainer.step()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        log(f"epoch {epoch + 1}/{cfg.train.epoch.nrof_epochs}  triplet loss {trainer.loss_value():.4f}  "
            f"{3 * nrof_triplets * cfg.train.epoch.size * world_size / dt:.1f} img/s")
        end_of_epoch(cfg, trainer, validation, epoch)
    return net, trainer


def dataset_pools(cfg, log=print, **kw):
    """P x K batches from cfg.dataset.path: the reference's equal-batches sampler (dataset.py:46-101), 20 classes x 5 images.
    The image.random_* keys (train_softmax.yaml:85-91) augment them, drawn from a generator seeded by cfg.seed; logged once.
    dataset.resident (with resident_cache, resident_bytes): the same batches from a decoded copy of the set in device memory."""
    from facenet_amd import dataset
    loader = dataset.ImageLoader(config=cfg.image)
    dbase = dataset.Database(cfg.dataset)
    augment = dataset.Augmentation.from_config(cfg.image, cfg.seed)
    if augment is not None:
        log(f"augmentation: {augment}")
    store = None
    if cfg.dataset.resident:                                      # the decoded set in device memory
        from facenet_amd import resident
        store = resident.from_config(cfg.dataset, dbase, device=kw.get("device", "cuda"), log=log)
    kw.setdefault("processes", True)
    return dataset.pipeline_with_equal_batches(loader, dbase.classes, cfg, augment=augment, resident=store, **kw)


@click.command()
@click.option("--config", default=None, type=Path, help="Path to yaml config file with used options of the application.")
def main(**options):
    cfg = config_mod.load_config(options["config"])
    from facenet_amd import callbacks
    validation = callbacks.from_config(cfg)                      # None unless validate.dataset.path is set
    if cfg.dataset.path:
        pipe = dataset_pools(cfg)
        batch_mined = triplet_settings(cfg)[0] != "mined"         # the batch strategies mine by the sampler's own labels
        train_tripletloss(cfg, people_per_batch=cfg.nrof_classes_per_batch, images_per_person=cfg.nrof_examples_per_class,
                          pools=pipe if batch_mined else (images for images, _ in pipe), validation=validation)
    else:
        train_tripletloss(cfg, validation=validation)


if __name__ == "__main__":
    main()
