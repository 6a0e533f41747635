# coding:utf-8
"""Write the embeddings of an image data set, the input of apps/train_classifier: apps/embeddings.py of the reference,
``python -m facenet_amd.apps.embeddings --config x.yaml``.

Database(dataset) -> FaceNet(model).evaluate per batch -> ``outfile``, an .npz with ``embeddings`` fp32 [N, E], ``labels``
int64 [N] and ``files`` [N].  The reference writes .h5 or TFRecord; neither library is used here, so such an ``outfile``
raises ValueError.  Without ``model.path`` the network keeps its initial weights."""
from __future__ import annotations

import random
from pathlib import Path

import click
import numpy as np
import torch

from facenet_amd.config import Config, _merge

DEFAULTS = {   # apps/configs/embeddings.yaml of the reference, with an .npz output
    "seed": 0,
    "batch_size": 100,
    "image": {"size": 160, "normalization": 0},
    "dataset": {"path": "~/datasets/vggface2/test_extracted_160", "nrof_classes": None, "min_nrof_images": None,
                "max_nrof_images": None},
    "model": {"path": None, "normalize": False},
    "outfile": None,
}


def load_options(path=None, overrides: dict = None) -> Config:
    """DEFAULTS <- yaml <- overrides.  ``outfile`` defaults to <dataset.path>_<model stem>/embeddings.npz (config.py:199-222 of
    the reference); log.txt goes beside it."""
    cfg = dict(DEFAULTS)
    if path is not None:
        import yaml
        with open(Path(path).expanduser()) as f:
            cfg = _merge(cfg, yaml.safe_load(f) or {})
    if overrides:
        cfg = _merge(cfg, overrides)
    c = Config(cfg)
    if c.outfile:
        c.outfile = Path(c.outfile).expanduser()
    else:
        stem = Path(c.model.path).stem if c.model.path else "model"
        c.outfile = Path(str(Path(c.dataset.path).expanduser()) + "_" + stem) / "embeddings.npz"
    if c.outfile.suffix in (".h5", ".tfrecord"):
        raise ValueError(f"{c.outfile}: .h5 and TFRecord outputs need h5py / TensorFlow, which this project does not use; "
                         "write an .npz")
    if c.outfile.suffix != ".npz":
        raise ValueError(f"{c.outfile}: the embeddings file must be an .npz")
    c.logfile = c.outfile.parent / "log.txt"
    random.seed(c.seed)
    np.random.seed(c.seed)
    return c


def write_embeddings(options, log=print):
    from facenet_amd import dataset
    from facenet_amd.api import FaceNet
    from facenet_amd.apps.train_classifier import write_text_log
    from facenet_amd.facenet import evaluate_embeddings

    options.outfile.parent.mkdir(parents=True, exist_ok=True)
    dbase = dataset.Database(options.dataset)
    write_text_log(options.logfile, dbase)
    log(dbase)

    model_cfg = Config(options.model.as_dict)
    model_cfg.image = options.image
    facenet = FaceNet(model_cfg)
    loader = dataset.ImageLoader(config=options.image)
    batches = dbase.tf_dataset_api(loader=loader, batch_size=options.batch_size)
    host_labels = ((images, labels.cpu() if torch.is_tensor(labels) else labels) for images, labels in batches)
    embeddings, labels = evaluate_embeddings(facenet.evaluate, host_labels)

    np.savez(options.outfile, embeddings=np.asarray(embeddings, dtype=np.float32), labels=np.asarray(labels, dtype=np.int64),
             files=np.asarray([str(f) for f in dbase.files]))
    log(f"output file: {options.outfile}")
    log(f"number of examples: {dbase.nrof_images}")
    return options.outfile


@click.command()
@click.option("--config", default=None, type=Path, help="Path to yaml config file with used options for the application.")
def main(**options):
    write_embeddings(load_options(options["config"]))


if __name__ == "__main__":
    main()
