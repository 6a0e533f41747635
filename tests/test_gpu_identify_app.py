"""FacePipeline.identify and `python -m facenet_amd.apps.identify` end to end on a two-photograph data set (the synthetic detector
and the untrained network of tests/test_gpu_face_crop.py).  The gallery holds the same photographs' own face embeddings, so every
face's nearest row is itself, at the distance the oracle gives for that pair."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch
from PIL import Image

from facenet_amd.detectors.face_detector import FaceDetector
from oracle import mtcnn_oracle as mo
from tests import identify_oracle as io

pytestmark = pytest.mark.gpu
FACE_BIAS = (0.5, 1.0, 1.0)     # the synthetic detector of tests/test_gpu_mtcnn.py: every stage passes some candidates


def _frame(h, w, seed=0, cell=8):
    """Blocky random image + noise (the frame of tests/test_gpu_mtcnn.py)."""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (-(-h // cell), -(-w // cell), 3), dtype=np.uint8)
    img = np.kron(base, np.ones((cell, cell, 1), np.uint8))[:h, :w].astype(np.int32) + rng.integers(-12, 13, (h, w, 3))
    return np.clip(img, 0, 255).astype(np.uint8)


@pytest.fixture(scope="module")
def detector(tmp_path_factory):
    path = tmp_path_factory.mktemp("mtcnn") / "w.npz"
    np.savez(path, **mo.random_weights(0, face_bias=FACE_BIAS))
    return FaceDetector(detector="pypimtcnn", weights_file=str(path)), str(path)


@pytest.fixture(scope="module")
def pipeline(detector):
    from facenet_amd.api import FaceNet
    from facenet_amd.config import Config
    from facenet_amd.recognize import FacePipeline
    facenet = FaceNet(Config({"normalize": True, "embedding_size": 128, "image": {"size": 160, "normalization": 0}}))
    return FacePipeline(detector[0], facenet, SimpleNamespace(size=160, margin=0.25))


@pytest.fixture(scope="module")
def photos(tmp_path_factory, pipeline):
    """Two photographs with faces and one without, in two class directories, and the gallery .npz of their own faces."""
    root = tmp_path_factory.mktemp("data")
    frames = {("alice", "a.png"): _frame(120, 160, seed=1), ("bob", "b.png"): _frame(97, 131, seed=4),
              ("bob", "tiny.png"): np.zeros((11, 30, 3), np.uint8)}          # smaller than one 12x12 cell at every scale
    emb, labels, files, per_photo = [], [], [], []
    for label, ((cls, name), frame) in enumerate(frames.items()):
        (root / "photos" / cls).mkdir(parents=True, exist_ok=True)
        Image.fromarray(frame).save(root / "photos" / cls / name)
        faces = pipeline.faces(frame)
        per_photo.append(len(faces))
        for _, e in faces:
            emb.append(e)
            labels.append(min(label, 1))
            files.append(str(root / "photos" / cls / name))
    assert per_photo[0] > 1 and per_photo[1] > 0 and per_photo[2] == 0
    np.savez(root / "gallery.npz", embeddings=np.asarray(emb, np.float32), labels=np.asarray(labels, np.int64), files=np.asarray(files))
    return SimpleNamespace(root=root, frames=list(frames.values()), emb=np.asarray(emb, np.float32), labels=np.asarray(labels),
                           files=files, per_photo=per_photo)


def test_face_pipeline_identify(pipeline, photos, monkeypatch):
    from facenet_amd.recognize import Gallery
    gallery = Gallery.from_file(photos.root / "gallery.npz")
    assert gallery.names == {0: "alice", 1: "bob"} and gallery.nrof_images == sum(photos.per_photo)
    ref = io.search(photos.emb, photos.emb, 1)
    assert np.array_equal(ref["rows"][:, 0], np.arange(len(photos.emb)))                  # every face's nearest row is itself
    seen = []
    monkeypatch.setattr(gallery, "_search", lambda q, *a: seen.append(q) or Gallery._search(gallery, q, *a))
    row = 0
    for frame, count in zip(photos.frames[:2], photos.per_photo):
        found = pipeline.identify(frame, gallery)
        boxes = pipeline.detector.detect(frame)
        assert len(found) == count and [b.info() for b, _ in found] == [b.info() for b in boxes]
        for _, (label, name, distance, near) in found:
            assert near == row and label == photos.labels[row] and name == ("alice", "bob")[label]
            assert np.float32(distance) == ref["dist"][row, 0]                            # the oracle's distance of the pair
            row += 1
    assert len(seen) == 2 and all(torch.is_tensor(q) and q.is_cuda and q.dtype == torch.float32 for q in seen)    # no host round trip
    # an unreachable threshold: everybody is unknown; nothing detected: no network and no search launch
    assert all(who[0] == -1 and who[1] is None for _, who in pipeline.identify(photos.frames[0], gallery, threshold=0.0))

    def no_launch(*a, **k):
        raise AssertionError("a launch without a face")
    monkeypatch.setattr(pipeline.facenet, "evaluate_device", no_launch)
    monkeypatch.setattr(gallery, "_search", no_launch)
    assert pipeline.identify(photos.frames[2], gallery) == []


def test_identify_app(detector, photos, tmp_path):
    """`python -m facenet_amd.apps.identify --config x.yaml` (entered through its click command)."""
    import yaml
    from click.testing import CliRunner

    from facenet_amd.apps import identify as app
    cfg, out = tmp_path / "x.yaml", tmp_path / "result" / "who.npz"
    k = 3
    cfg.write_text(yaml.safe_dump({"dataset": {"path": str(photos.root / "photos")}, "model": {"normalize": True, "embedding_size": 128},
                                   "image": {"size": 160, "margin": 0.25}, "mtcnn": {"weights_file": detector[1]},
                                   "gallery": {"path": str(photos.root / "gallery.npz")}, "identify": {"k": k}, "file": str(out)}))
    result = CliRunner().invoke(app.main, ["--config", str(cfg)], catch_exceptions=False)
    assert result.exit_code == 0, result.output
    z = np.load(out)
    n = sum(photos.per_photo)
    assert sorted(z.files) == sorted(["files", "face", "boxes", "confidence", "labels", "names", "distances", "rows"])
    assert [str(f) for f in z["files"]] == photos.files                                   # tiny.png contributes no row
    assert z["face"].tolist() == [i for c in photos.per_photo for i in range(c)]
    assert z["boxes"].shape == (n, 4) and z["boxes"].dtype == np.int64 and z["confidence"].shape == (n,)
    assert z["labels"].shape == (n,) and z["labels"].dtype == np.int64 and z["names"].shape == (n,)
    assert z["distances"].shape == (n, k) and z["distances"].dtype == np.float32
    assert z["rows"].shape == (n, k) and z["rows"].dtype == np.int32
    ref = io.search(photos.emb, photos.emb, k)
    assert np.array_equal(z["rows"], ref["rows"]) and np.array_equal(z["rows"][:, 0], np.arange(n))
    assert np.array_equal(z["distances"], ref["dist"])
    assert np.array_equal(z["labels"], photos.labels) and z["names"].tolist() == [("alice", "bob")[c] for c in photos.labels]
    assert sum("gallery row" in line for line in result.output.splitlines()) == n          # one line per face
