# coding:utf-8
"""Embeddings of every face in every photograph of a data set, detector -> crop -> network on the device (FacePipeline,
DESIGN.md section 17): ``python -m facenet_amd.apps.photo_embeddings --config x.yaml``.

Keys: dataset.path, model.* as in apps/embeddings.py, image.size, image.margin, image.align (landmark alignment instead of the box
crop; off when absent), detector, mtcnn.weights_file, file.  Every image
of the data set is read, and its faces go to ``file``, one .npz with a row per face: ``files`` (the photograph), ``face`` (the
index within the photograph), ``boxes`` int64 [N, 4] = left, top, width, height, ``confidence`` float64 [N] and ``embeddings``
float32 [N, E].  Images without a face, and files that cannot be read, contribute no row."""
from __future__ import annotations

from pathlib import Path

import click
import numpy as np
from PIL import Image

from facenet_amd.config import Config, _merge

DEFAULTS = {
    "image": {"size": 160, "margin": 0.14, "normalization": 0},
    "dataset": {"path": None, "nrof_classes": None, "min_nrof_images": None, "max_nrof_images": None},
    "model": {"path": None, "normalize": True},
    "detector": "pypimtcnn",
    "mtcnn": {"weights_file": None},
    "file": None,
}


def load_options(path=None, overrides: dict = None) -> Config:
    """DEFAULTS <- yaml <- overrides.  ``file`` defaults to <dataset.path>_<model stem>/photo_embeddings.npz."""
    cfg = dict(DEFAULTS)
    if path is not None:
        import yaml
        with open(Path(path).expanduser()) as f:
            cfg = _merge(cfg, yaml.safe_load(f) or {})
    if overrides:
        cfg = _merge(cfg, overrides)
    c = Config(cfg)
    if not c.dataset.path:
        raise ValueError("photo_embeddings: dataset.path is not specified")
    if c.file:
        c.file = Path(c.file).expanduser()
    else:
        stem = Path(c.model.path).stem if c.model.path else "model"
        c.file = Path(str(Path(c.dataset.path).expanduser()) + "_" + stem) / "photo_embeddings.npz"
    if c.file.suffix != ".npz":
        raise ValueError(f"{c.file}: the output file must be an .npz")
    return c


def build_pipeline(options):
    from facenet_amd.api import FaceNet
    from facenet_amd.detectors.face_detector import FaceDetector
    from facenet_amd.recognize import FacePipeline
    detector = FaceDetector(detector=options.detector if options.detector else "pypimtcnn", weights_file=options.mtcnn.weights_file)
    model_cfg = Config(options.model.as_dict)
    model_cfg.image = Config({"size": options.image.size, "normalization": options.image.normalization or 0})
    return FacePipeline(detector, FaceNet(model_cfg), options.image, align=bool(options.image.align))


def write_photo_embeddings(options, pipeline=None, log=print):
    """pipeline: anything with `.faces(uint8 [H, W, 3]) -> [(BoundingBox, embedding)]` and `.detector.mode` (FacePipeline)."""
    from facenet_amd import dataset

    dbase = dataset.Database(options.dataset)
    log(dbase)
    pipeline = build_pipeline(options) if pipeline is None else pipeline
    files, face, boxes, confidence, embeddings, unread = [], [], [], [], [], 0
    for path in dbase.files:
        try:
            pixels = np.asarray(Image.open(path).convert(pipeline.detector.mode), dtype=np.uint8)
        except Exception:
            unread += 1
            continue
        for n, (box, emb) in enumerate(pipeline.faces(pixels)):
            files.append(str(path))
            face.append(n)
            boxes.append([box.left, box.top, box.width, box.height])
            confidence.append(np.nan if box.confidence is None else float(box.confidence))
            embeddings.append(np.asarray(emb, dtype=np.float32))
    options.file.parent.mkdir(parents=True, exist_ok=True)
    width = embeddings[0].shape[0] if embeddings else 0
    np.savez(options.file, files=np.asarray(files, dtype=str), face=np.asarray(face, dtype=np.int64),
             boxes=np.asarray(boxes, dtype=np.int64).reshape(-1, 4), confidence=np.asarray(confidence, dtype=np.float64),
             embeddings=np.asarray(embeddings, dtype=np.float32).reshape(-1, width))
    log('Number of files that cannot be read', unread)
    log(f"output file: {options.file}")
    log(f"number of faces: {len(files)} in {dbase.nrof_images} images")
    return options.file


@click.command()
@click.option("--config", default=None, type=Path, help="Path to yaml config file with used options for the application.")
def main(**options):
    write_photo_embeddings(load_options(options["config"]))


if __name__ == "__main__":
    main()
