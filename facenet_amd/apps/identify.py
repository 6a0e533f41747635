# coding:utf-8
"""Who is in every photograph of a data set: detector -> crop -> network -> gallery search on the device (FacePipeline.identify,
DESIGN.md section 19): ``python -m facenet_amd.apps.identify --config x.yaml``.

Keys: those of apps/photo_embeddings.py (dataset.path, model.*, image.size, image.margin, image.align, detector, mtcnn.weights_file, file)
and gallery.path (required: the .npz of apps/embeddings.py with the known faces), gallery.metric (0 or 1), identify.k (neighbours
kept per face, 1..64) and at most one of identify.threshold (a number) and identify.classifier (an .npz written by a
FaceToFaceNormalizedEmbeddingsClassifier's ``save``); with neither every face gets its nearest gallery row's label.
identify.nlist (``--nlist``; unset: off) searches through an inverted-file index of that many k-means lists (at most one per
gallery row), built once from the gallery (Gallery.ivf), of which every face probes identify.nprobe (``--nprobe``, default 8).
identify.quantized (``--quantized``; default off) searches through int8 codes of the gallery (Gallery.quantize, DESIGN.md section
27) with a shortlist of identify.shortlist rows (``--shortlist``, k..64, default 64); the answers are the exhaustive search's bit
for bit.  It cannot be combined with identify.nlist.  identify.templates (``--templates``; default off) searches one template
per identity, the normalised mean of its gallery rows (Gallery.templates), instead of the rows: ``rows`` are
then rows of the template gallery, one per label in ascending label order.  It cannot be combined with identify.nlist or
identify.quantized.  identify.candidates (``--candidates``, 1..64; unset: off) adds every face's candidate list of that many
distinct identities (Gallery.candidates): ``candidate_labels`` int64 [N, c], ``candidate_distances`` float32 [N, c] and
``candidate_rows`` int32 [N, c] (each identity's nearest gallery row; -1 / inf / -1 where the gallery has fewer identities), which
needs the exhaustive search and so cannot be combined with identify.nlist either.  Every image
of the data set is read and its faces go to ``file``, one .npz with a row per face: ``files``, ``face``, ``boxes`` int64 [N, 4],
``confidence`` float64 [N] as photo_embeddings writes them, ``labels`` int64 [N] (-1: nobody nearer than the threshold),
``names`` [N] ('' for -1 or a gallery without names), ``distances`` float32 [N, k] and ``rows`` int32 [N, k] (gallery rows by
ascending distance; -1 / inf where the gallery has fewer than k rows).  One line is logged per face."""
from __future__ import annotations

from pathlib import Path

import click
import numpy as np
from PIL import Image

from facenet_amd.apps import photo_embeddings
from facenet_amd.config import Config, _merge

DEFAULTS = dict(photo_embeddings.DEFAULTS, gallery={"path": None, "metric": 0},
                identify={"threshold": None, "classifier": None, "k": 1, "nlist": None, "nprobe": None, "quantized": False,
                          "shortlist": None, "candidates": None, "templates": False})


def load_options(path=None, overrides: dict = None) -> Config:
    """DEFAULTS <- yaml <- overrides.  ``file`` defaults to <dataset.path>_<model stem>/identified.npz."""
    cfg = dict(DEFAULTS)
    if path is not None:
        import yaml
        with open(Path(path).expanduser()) as f:
            cfg = _merge(cfg, yaml.safe_load(f) or {})
    if overrides:
        cfg = _merge(cfg, overrides)
    c = Config(cfg)
    if not c.dataset.path:
        raise ValueError("identify: dataset.path is not specified")
    if not c.gallery.path:
        raise ValueError("identify: gallery.path is not specified")
    c.gallery.path = Path(c.gallery.path).expanduser()
    if c.gallery.metric not in (0, 1):
        raise ValueError("Undefined similarity metric {}".format(c.gallery.metric))
    if c.identify.threshold is not None and c.identify.classifier is not None:
        raise ValueError("identify: give identify.threshold or identify.classifier, not both")
    if c.identify.classifier is not None:
        c.identify.classifier = Path(c.identify.classifier).expanduser()
    if not isinstance(c.identify.k, int) or not 1 <= c.identify.k <= 64:
        raise ValueError(f"identify.k must be an integer in [1, 64], got {c.identify.k!r}")
    for key in ("nlist", "nprobe"):
        value = getattr(c.identify, key)
        if value is not None and (isinstance(value, bool) or not isinstance(value, int) or value < 1):
            raise ValueError(f"identify.{key} must be an integer of at least 1, got {value!r}")
    if c.identify.nprobe is not None and c.identify.nlist is None:
        raise ValueError("identify.nprobe needs identify.nlist")
    if not isinstance(c.identify.quantized, bool):
        raise ValueError(f"identify.quantized must be true or false, got {c.identify.quantized!r}")
    if c.identify.quantized and c.identify.nlist is not None:
        raise ValueError("identify.quantized cannot be combined with identify.nlist: quantised inverted-file lists are not built")
    shortlist = c.identify.shortlist
    if shortlist is not None:
        if not c.identify.quantized:
            raise ValueError("identify.shortlist needs identify.quantized")
        if isinstance(shortlist, bool) or not isinstance(shortlist, int) or not c.identify.k <= shortlist <= 64:
            raise ValueError(f"identify.shortlist must be an integer in [identify.k, 64], got {shortlist!r}")
    candidates = c.identify.candidates
    if candidates is not None and (isinstance(candidates, bool) or not isinstance(candidates, int) or not 1 <= candidates <= 64):
        raise ValueError(f"identify.candidates must be an integer in [1, 64], got {candidates!r}")
    if candidates is not None and c.identify.nlist is not None:
        raise ValueError("identify.candidates cannot be combined with identify.nlist: candidate lists need the exhaustive search")
    if not isinstance(c.identify.templates, bool):
        raise ValueError(f"identify.templates must be true or false, got {c.identify.templates!r}")
    if c.identify.templates and (c.identify.nlist is not None or c.identify.quantized):
        raise ValueError("identify.templates cannot be combined with identify.nlist or identify.quantized: "
                         "the templates are searched exhaustively in fp32")
    if c.file:
        c.file = Path(c.file).expanduser()
    else:
        stem = Path(c.model.path).stem if c.model.path else "model"
        c.file = Path(str(Path(c.dataset.path).expanduser()) + "_" + stem) / "identified.npz"
    if c.file.suffix != ".npz":
        raise ValueError(f"{c.file}: the output file must be an .npz")
    return c


def load_gallery(options):
    """(Gallery, fp32 threshold or None) of the options."""
    from facenet_amd.faceclass import FaceToFaceNormalizedEmbeddingsClassifier
    from facenet_amd.recognize import Gallery
    gallery = Gallery.from_file(options.gallery.path, metric=options.gallery.metric)
    classifier = None
    if options.identify.classifier is not None:
        classifier = FaceToFaceNormalizedEmbeddingsClassifier().load(options.identify.classifier)
    threshold = gallery.threshold_of(options.identify.threshold, classifier)
    if options.identify.templates:
        gallery = gallery.templates()
    if options.identify.nlist is not None:
        gallery = gallery.ivf(min(options.identify.nlist, gallery.nrof_images))
        if options.identify.nprobe is not None:
            gallery.nprobe = options.identify.nprobe
    if options.identify.quantized:
        gallery = gallery.quantize(64 if options.identify.shortlist is None else options.identify.shortlist)
    return gallery, threshold


def write_identified(options, pipeline=None, gallery=None, threshold=None, log=print):
    """pipeline: a FacePipeline (built from the options when None); gallery / threshold: as `load_gallery` returns them."""
    from facenet_amd import dataset

    dbase = dataset.Database(options.dataset)
    log(dbase)
    pipeline = photo_embeddings.build_pipeline(options) if pipeline is None else pipeline
    if gallery is None:
        gallery, threshold = load_gallery(options)
    log(gallery)
    k, nc = options.identify.k, options.identify.candidates
    candidates = {"candidate_labels": [], "candidate_distances": [], "candidate_rows": []}
    files, face, boxes, confidence, labels, names, distances, rows, unread = [], [], [], [], [], [], [], [], 0
    for path in dbase.files:
        try:
            pixels = np.asarray(Image.open(path).convert(pipeline.detector.mode), dtype=np.uint8)
        except Exception:
            unread += 1
            continue
        found, crops = pipeline.crops(pixels)
        if len(found) == 0:
            continue
        emb = pipeline.embed_device(crops)
        dist, near = (t.cpu().numpy() for t in gallery.search(emb, k=k))
        if nc is not None:
            cdist, crows, clabels = (t.cpu().numpy() for t in gallery.candidates(emb, k=nc))
            candidates["candidate_labels"].append(clabels)
            candidates["candidate_distances"].append(cdist)
            candidates["candidate_rows"].append(crows)
        for n, box in enumerate(found):
            label, name, _, _ = gallery.who(dist[n, 0], near[n, 0], threshold)
            name = "" if name is None else str(name)
            files.append(str(path))
            face.append(n)
            boxes.append([box.left, box.top, box.width, box.height])
            confidence.append(np.nan if box.confidence is None else float(box.confidence))
            labels.append(label)
            names.append(name)
            distances.append(dist[n])
            rows.append(near[n])
            log(f"{path} face {n}: {name or label} distance {dist[n, 0]:.6f} gallery row {near[n, 0]}")
    extra = {}
    if nc is not None:
        for (name, parts), dtype in zip(candidates.items(), (np.int64, np.float32, np.int32)):
            extra[name] = np.concatenate(parts + [np.empty((0, nc), dtype=dtype)]).astype(dtype)
    options.file.parent.mkdir(parents=True, exist_ok=True)
    np.savez(options.file, files=np.asarray(files, dtype=str), face=np.asarray(face, dtype=np.int64),
             boxes=np.asarray(boxes, dtype=np.int64).reshape(-1, 4), confidence=np.asarray(confidence, dtype=np.float64),
             labels=np.asarray(labels, dtype=np.int64), names=np.asarray(names, dtype=str),
             distances=np.asarray(distances, dtype=np.float32).reshape(-1, k), rows=np.asarray(rows, dtype=np.int32).reshape(-1, k), **extra)
    log('Number of files that cannot be read', unread)
    log(f"output file: {options.file}")
    log(f"number of faces: {len(files)} in {dbase.nrof_images} images")
    return options.file


@click.command()
@click.option("--config", default=None, type=Path, help="Path to yaml config file with used options for the application.")
@click.option("--nlist", default=None, type=int, help="Search through an inverted-file index of this many lists (identify.nlist).")
@click.option("--nprobe", default=None, type=int, help="Lists every face probes (identify.nprobe); needs --nlist or identify.nlist.")
@click.option("--quantized", is_flag=True, default=None, help="Search through int8 codes of the gallery (identify.quantized).")
@click.option("--shortlist", default=None, type=int, help="Rows the int8 stage keeps per face (identify.shortlist); needs --quantized.")
@click.option("--candidates", default=None, type=int, help="Distinct identities listed per face (identify.candidates), 1..64.")
@click.option("--templates", is_flag=True, default=None, help="Search one mean template per identity (identify.templates).")
def main(**options):
    given = {key: options[key] for key in ("nlist", "nprobe", "quantized", "shortlist", "candidates", "templates") if options[key] is not None}
    write_identified(load_options(options["config"], {"identify": given} if given else None))


if __name__ == "__main__":
    main()
