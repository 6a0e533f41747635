# coding:utf-8
"""Which faces are the same person: DBSCAN over face embeddings on the device (Gallery.cluster):
``python -m facenet_amd.apps.cluster --config x.yaml``.

Input, exactly one of: embeddings.path (the .npz of apps/embeddings.py: ``embeddings``, optionally ``labels`` / ``files``) or
dataset.path (photographs; with the keys of apps/photo_embeddings.py: model.*, image.size, image.margin, image.align, detector,
mtcnn.weights_file, every face goes detector -> crop -> network -> clustering on the device).  cluster.metric (0 or 1), exactly
one of cluster.threshold (a number) and cluster.classifier (an .npz written by a FaceToFaceNormalizedEmbeddingsClassifier's
``save``), cluster.min_samples (>= 1; 1 is single linkage at the threshold).  ``file`` receives one .npz with a row per face:
``files`` ('' without file names), ``labels`` int64 [N] (the cluster, -1 for noise), ``core`` bool [N], and from photographs
``face`` (the index within the photograph) and ``boxes`` int64 [N, 4] = left, top, width, height.  The cluster count, the noise
count and, when the input carries true labels (the .npz's ``labels``; the class directory of a photograph), the pairwise
precision, recall and F are logged.

cluster.method: ``dbscan`` (the default, all of the above) or ``hdbscan`` (Gallery.hdbscan, DESIGN.md section 30: no threshold, so
cluster.threshold and cluster.classifier must be absent, and cluster.metric must be 0), with cluster.min_cluster_size (>= 2, default
5) and cluster.min_samples (absent: cluster.min_cluster_size); the .npz then holds ``probabilities`` float64 [N] in place of
``core``."""
from __future__ import annotations

from pathlib import Path

import click
import numpy as np
from PIL import Image

from facenet_amd.apps import photo_embeddings
from facenet_amd.config import Config, _merge

DEFAULTS = dict(photo_embeddings.DEFAULTS, embeddings={"path": None},
                cluster={"threshold": None, "classifier": None, "min_samples": 1, "metric": 0, "method": "dbscan", "min_cluster_size": 5})


def load_options(path=None, overrides: dict = None) -> Config:
    """DEFAULTS <- yaml <- overrides.  ``file`` defaults to clusters.npz next to the embeddings file, or to
    <dataset.path>_<model stem>/clusters.npz."""
    cfg = dict(DEFAULTS)
    if path is not None:
        import yaml
        with open(Path(path).expanduser()) as f:
            cfg = _merge(cfg, yaml.safe_load(f) or {})
    if overrides:
        cfg = _merge(cfg, overrides)
    c = Config(cfg)
    if bool(c.embeddings.path) == bool(c.dataset.path):
        raise ValueError("cluster: give embeddings.path (an .npz of embeddings) or dataset.path (photographs), one of them")
    if c.cluster.metric not in (0, 1):
        raise ValueError("Undefined similarity metric {}".format(c.cluster.metric))
    if c.cluster.method not in ("dbscan", "hdbscan"):
        raise ValueError(f"cluster.method must be 'dbscan' or 'hdbscan', got {c.cluster.method!r}")
    if c.cluster.method == "hdbscan":
        return _hdbscan_options(c, path, overrides)
    if (c.cluster.threshold is None) == (c.cluster.classifier is None):
        raise ValueError("cluster: give cluster.threshold or cluster.classifier, one of them: clustering has no closed set")
    if c.cluster.classifier is not None:
        c.cluster.classifier = Path(c.cluster.classifier).expanduser()
    if isinstance(c.cluster.min_samples, bool) or not isinstance(c.cluster.min_samples, int) or c.cluster.min_samples < 1:
        raise ValueError(f"cluster.min_samples must be an integer of at least 1, got {c.cluster.min_samples!r}")
    return _output_file(c)


def _given(path, overrides, key):
    """Whether the yaml file or the overrides set cluster.<key> (the merged options cannot tell a default from a given value)."""
    given = False
    if path is not None:
        import yaml
        with open(Path(path).expanduser()) as f:
            given = key in ((yaml.safe_load(f) or {}).get("cluster") or {})
    return given or key in ((overrides or {}).get("cluster") or {})


def _hdbscan_options(c, path, overrides):
    if c.cluster.threshold is not None or c.cluster.classifier is not None:
        raise ValueError("cluster: cluster.method 'hdbscan' takes no cluster.threshold and no cluster.classifier: it needs no threshold")
    if c.cluster.metric != 0:
        raise ValueError("cluster: cluster.method 'hdbscan' needs cluster.metric 0, got {}".format(c.cluster.metric))
    size = c.cluster.min_cluster_size
    if isinstance(size, bool) or not isinstance(size, int) or size < 2:
        raise ValueError(f"cluster.min_cluster_size must be an integer of at least 2, got {size!r}")
    if not _given(path, overrides, "min_samples"):
        c.cluster.min_samples = size                         # as scikit-learn: min_samples defaults to min_cluster_size
    if isinstance(c.cluster.min_samples, bool) or not isinstance(c.cluster.min_samples, int) or c.cluster.min_samples < 1:
        raise ValueError(f"cluster.min_samples must be an integer of at least 1, got {c.cluster.min_samples!r}")
    return _output_file(c)


def _output_file(c):
    if c.embeddings.path:
        c.embeddings.path = Path(c.embeddings.path).expanduser()
    if c.file:
        c.file = Path(c.file).expanduser()
    elif c.embeddings.path:
        c.file = c.embeddings.path.parent / "clusters.npz"
    else:
        stem = Path(c.model.path).stem if c.model.path else "model"
        c.file = Path(str(Path(c.dataset.path).expanduser()) + "_" + stem) / "clusters.npz"
    if c.file.suffix != ".npz":
        raise ValueError(f"{c.file}: the output file must be an .npz")
    return c


def _photographs(options, pipeline, log):
    """-> (Clustering or None, files, truth, face, boxes) of every face of the data set's photographs."""
    from facenet_amd import dataset

    dbase = dataset.Database(options.dataset)
    log(dbase)
    pipeline = photo_embeddings.build_pipeline(options) if pipeline is None else pipeline
    paths, frames, unread = [], [], 0
    for path in dbase.files:
        try:
            frames.append(np.asarray(Image.open(path).convert(pipeline.detector.mode), dtype=np.uint8))
            paths.append(path)
        except Exception:
            unread += 1
    log('Number of files that cannot be read', unread)
    clustering, faces = pipeline.cluster(frames, metric=options.cluster.metric, **_cluster_arguments(options))
    files = [str(paths[i]) for i, _, _ in faces]
    truth = np.unique([Path(f).parent.name for f in files], return_inverse=True)[1] if files else None
    boxes = np.asarray([[b.left, b.top, b.width, b.height] for _, _, b in faces], dtype=np.int64).reshape(-1, 4)
    return clustering, files, truth, np.asarray([n for _, n, _ in faces], dtype=np.int64), boxes


def _cluster_arguments(options):
    if options.cluster.method == "hdbscan":
        return {"method": "hdbscan", "min_cluster_size": options.cluster.min_cluster_size, "min_samples": options.cluster.min_samples}
    if options.cluster.classifier is None:
        return {"threshold": options.cluster.threshold, "min_samples": options.cluster.min_samples}
    from facenet_amd.faceclass import FaceToFaceNormalizedEmbeddingsClassifier
    classifier = FaceToFaceNormalizedEmbeddingsClassifier().load(options.cluster.classifier)
    return {"classifier": classifier, "min_samples": options.cluster.min_samples}


def write_clusters(options, pipeline=None, log=print):
    """pipeline: a FacePipeline for the photographs of dataset.path (built from the options when None)."""
    from facenet_amd.recognize import Gallery
    from facenet_amd.statistics import pairwise_clustering_scores

    extra = {}
    if options.embeddings.path:
        gallery = Gallery.from_file(options.embeddings.path, metric=options.cluster.metric)
        log(gallery)
        with np.load(options.embeddings.path) as f:
            truth = np.asarray(f["labels"]) if "labels" in f else None
        files = [""] * gallery.nrof_images if gallery.files is None else gallery.files.tolist()
        arguments = _cluster_arguments(options)
        clustering = gallery.hdbscan(**arguments) if arguments.pop("method", "dbscan") == "hdbscan" else gallery.cluster(**arguments)
    else:
        clustering, files, truth, extra["face"], extra["boxes"] = _photographs(options, pipeline, log)
    labels = np.zeros(0, np.int64) if clustering is None else clustering.labels
    if options.cluster.method == "hdbscan":
        extra["probabilities"] = np.zeros(0, np.float64) if clustering is None else clustering.probabilities
    else:
        extra["core"] = np.zeros(0, bool) if clustering is None else clustering.core
    options.file.parent.mkdir(parents=True, exist_ok=True)
    np.savez(options.file, files=np.asarray(files, dtype=str), labels=labels, **extra)
    log(f"output file: {options.file}")
    log(f"number of faces: {len(labels)}")
    log(f"number of clusters: {0 if clustering is None else clustering.nrof_clusters}")
    log(f"number of noise faces: {int(np.count_nonzero(labels < 0))}")
    if truth is not None and len(labels):
        log("pairwise precision {:1.5f} recall {:1.5f} F {:1.5f}".format(*pairwise_clustering_scores(truth, labels)))
    return options.file


@click.command()
@click.option("--config", default=None, type=Path, help="Path to yaml config file with used options for the application.")
def main(**options):
    write_clusters(load_options(options["config"]))


if __name__ == "__main__":
    main()
