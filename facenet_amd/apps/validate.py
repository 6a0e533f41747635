# coding:utf-8
"""Validate a face recognizer: apps/validate.py of the reference, ``python -m facenet_amd.apps.validate --config x.yaml``.

Database(dataset) -> FaceNet(model) with ``normalize = True`` -> embeddings of every image -> FaceToFaceValidation.  The data
set, the embeddings' shape, the report and the elapsed time are printed and appended to ``file`` (default
``<model.path>/report.txt``), in the layout of the reference's models/*/report.txt."""
from __future__ import annotations

import random
import time
from pathlib import Path

import click
import numpy as np
import torch

from facenet_amd.config import Config, _merge

DEFAULTS = {   # apps/configs/validate.yaml of the reference
    "seed": 0,
    "batch_size": 100,
    "image": {"size": 160, "normalization": 0},
    "dataset": {"path": "~/datasets/vggface2/test_extracted_160", "h5file": None, "nrof_classes": None, "min_nrof_images": None,
                "max_nrof_images": None},
    "model": {"path": None},
    # validate.far_targets (not set here: absent means None): a list of false-accept rates; the exact VerificationCurve at these
    # rates is appended to the report.  validate.fpir_targets (likewise absent): a list of false-positive
    # identification rates, and validate.fpir_rank (default 1); the open-set IdentificationCurve at these rates follows (section 24).
    # validate.false_examples (likewise absent): {threshold: null, max_fneg: 10, max_fpos: 2, fpos_dir: null, fneg_dir: null}; the
    # worst pairs at the threshold (null: the mean of the folds' max-accuracy thresholds) are listed in the report and written as
    # pictures into the directories (null: false_positives and false_negatives next to the report) (section 28)
    "validate": {"nrof_folds": 10, "metric": 0, "far_target": 0.001},
    "file": None,
}


def load_options(path=None, overrides: dict = None) -> Config:
    """DEFAULTS <- yaml <- overrides; ``model.normalize`` is forced on (validate.py:20); ``file`` defaults to report.txt in the
    model's directory (``model.path`` itself when it is a directory, else the directory of the weights file)."""
    cfg = dict(DEFAULTS)
    if path is not None:
        import yaml
        with open(Path(path).expanduser()) as f:
            cfg = _merge(cfg, yaml.safe_load(f) or {})
    if overrides:
        cfg = _merge(cfg, overrides)
    c = Config(cfg)
    c.model.normalize = True
    if c.file:
        c.file = Path(c.file).expanduser()
    else:
        model = Path(c.model.path).expanduser() if c.model.path else Path(".")
        c.file = (model if model.is_dir() or not model.suffix else model.parent) / "report.txt"
    random.seed(c.seed)
    np.random.seed(c.seed)
    return c


def validate(options, log=print):
    """Returns the FaceToFaceValidation; ``options`` as ``load_options`` builds them.  ``report.curve`` is the VerificationCurve
    that ``validate.far_targets`` asks for and ``report.identification`` the IdentificationCurve that ``validate.fpir_targets`` asks
    for, each None without its key; ``report.false_examples`` likewise the FalseExamples of ``validate.false_examples``."""
    from facenet_amd import dataset
    from facenet_amd.api import FaceNet
    from facenet_amd.apps.train_classifier import write_text_log
    from facenet_amd.facenet import evaluate_embeddings
    from facenet_amd.statistics import FaceToFaceValidation, false_examples, identification_curve, verification_curve

    start = time.monotonic()
    options.file.parent.mkdir(parents=True, exist_ok=True)
    dbase = dataset.Database(options.dataset)
    write_text_log(options.file, dbase)
    log(dbase)

    model_cfg = Config(options.model.as_dict)
    model_cfg.image = options.image
    facenet = FaceNet(model_cfg)
    batches = dbase.tf_dataset_api(loader=dataset.ImageLoader(config=options.image), batch_size=options.batch_size)
    host_labels = ((images, labels.cpu() if torch.is_tensor(labels) else labels) for images, labels in batches)
    embeddings, labels = evaluate_embeddings(facenet.evaluate, host_labels)
    info = "EvaluationOfEmbeddings\nmodel: path: {}\n\nembedding size: {}\n".format(options.model.path, embeddings.shape)
    write_text_log(options.file, info)
    log(info)

    report = FaceToFaceValidation(embeddings, labels, options.validate)
    report.write_report(options.file)
    log(report)
    report.curve = verification_curve(embeddings, labels, options.validate)
    if report.curve is not None:
        write_text_log(options.file, report.curve)
        log(report.curve)
    report.identification = identification_curve(embeddings, labels, options.validate)
    if report.identification is not None:
        write_text_log(options.file, report.identification)
        log(report.identification)
    # rows are in the database's order, so row i is dbase.files[i]
    threshold = float(np.mean([m.threshold for m in report.reports[0].conf_matrix_test]))
    report.false_examples = false_examples(embeddings, labels, dbase.files, options.validate, threshold)
    if report.false_examples is not None:
        write_text_log(options.file, report.false_examples)
        log(report.false_examples)
        asked = options.validate.false_examples
        report.false_examples.write_false_pairs(asked.fpos_dir or options.file.parent / "false_positives",
                                                asked.fneg_dir or options.file.parent / "false_negatives")

    with options.file.open("at") as f:
        f.write("elapsed time: {:.3f}\n".format(time.monotonic() - start))
    log("Report has been written to the file {}".format(options.file))
    return report


@click.command()
@click.option("--config", default=None, type=Path, help="Path to yaml config file with used options for the application.")
def main(**options):
    validate(load_options(options["config"]))


if __name__ == "__main__":
    main()
