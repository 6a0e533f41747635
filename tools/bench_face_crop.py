"""The device face crop against the PIL route on the MI355X, for a 1280x720 frame with 1, 8 and 32 boxes of
about 200 pixels at image.size 160 and image.margin 0.14:

  (a) device route: frame already resident -> [F,160,160,3] on the device (image_processing_batch with the centre cut: the copy of
      the windows, the table launch and the resampling launch);
  (b) PIL route: image_processing per face + the centre cut + the host->device copy of the stack;
  (c) photo -> embeddings: FacePipeline.faces against the same sequence with the PIL route in the middle (detector on the host
      array, PIL crops, FaceNet.evaluate of the host stack at the same padded batch size).  The detector is the real MTCNN with synthetic weights; so that both
      routes embed the same F faces its boxes are replaced by the F fixed ones after it has run.

Every figure is the median over ROUNDS whole loops of a host clock around work that ends in a device synchronise, after warm-up
of every shape; (a) and (b), and the two routes of (c), alternate within a round.  (b) runs on the host: the CPUs this process
may use are printed with it.  One JSON line per figure."""
import json
import os
import statistics
import sys
import time
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import torch
from PIL import Image

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from facenet_amd.detectors.face_detector import BoundingBox, FaceDetector, image_processing, image_processing_batch

H, W, SIZE, MARGIN = 720, 1280, 160, 0.14
ROUNDS, WARMUP = 15, 3


def frame_and_boxes(count, seed=0):
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (H // 8, W // 8, 3), dtype=np.uint8)
    frame = np.kron(base, np.ones((8, 8, 1), np.uint8)).astype(np.int32) + rng.integers(-12, 13, (H, W, 3))
    boxes = [BoundingBox(int(rng.integers(0, W - 220)), int(rng.integers(0, H - 220)), int(rng.integers(180, 221)), int(rng.integers(180, 221)),
                         0.99) for _ in range(count)]
    return np.clip(frame, 0, 255).astype(np.uint8), boxes


def pil_route(img, boxes, opts, centre):
    thumbs = [np.asarray(image_processing(img, box, opts))[centre:centre + SIZE, centre:centre + SIZE] for box in boxes]
    return np.stack(thumbs)


def timed(fn, loops):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(loops):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / loops * 1e6


def compare(name, routes, loops, extra):
    """routes: {label: callable}; alternated within each round."""
    for fn in routes.values():
        for _ in range(WARMUP):
            fn()
    times = {label: [] for label in routes}
    for _ in range(ROUNDS):
        for label, fn in routes.items():
            times[label].append(timed(fn, loops))
    for label, t in times.items():
        print(json.dumps(dict(extra, measure=name, route=label, us_median=round(statistics.median(t), 1), us_min=round(min(t), 1),
                              us_max=round(max(t), 1), rounds=ROUNDS, loops_per_round=loops)), flush=True)
    return {label: statistics.median(t) for label, t in times.items()}


class FixedBoxes:
    """The detector runs on the frame it is given (its cost is part of both routes); the boxes it reports are the fixed ones."""

    def __init__(self, detector, boxes):
        self.detector, self.boxes, self.mode = detector, boxes, detector.mode

    def detect(self, image):
        self.detector.detect(image)
        return self.boxes


def main():
    from facenet_amd.api import FaceNet
    from facenet_amd.config import Config
    from facenet_amd.recognize import FacePipeline, padded_batch
    from oracle import mtcnn_oracle as mo
    assert torch.cuda.is_available(), "bench_face_crop needs the MI355X"
    opts = SimpleNamespace(size=SIZE, margin=MARGIN)
    cpus = len(os.sched_getaffinity(0))
    threads = os.environ.get("OMP_NUM_THREADS")
    print(json.dumps({"host_cpus_usable": cpus, "host_cpus_total": os.cpu_count(), "OMP_NUM_THREADS": threads,
                      "note": "the PIL route resizes one face at a time on one CPU thread"}), flush=True)
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        np.savez(Path(d) / "w.npz", **mo.random_weights(0, face_bias=(-0.3, 1.0, 1.0)))
        mtcnn = FaceDetector(detector="pypimtcnn", weights_file=str(Path(d) / "w.npz"))
    facenet = FaceNet(Config({"normalize": True, "embedding_size": 128, "image": {"size": SIZE, "normalization": 0}}))
    for count in (1, 8, 32):
        frame, boxes = frame_and_boxes(count)
        img, dev = Image.fromarray(frame), torch.from_numpy(frame).cuda()
        side = image_processing_batch(dev, boxes, opts).shape[1]
        centre = (side - SIZE) // 2
        same = np.array_equal(image_processing_batch(dev, boxes, opts, centre_crop=True).cpu().numpy(), pil_route(img, boxes, opts, centre))
        extra = {"faces": count, "frame": f"{W}x{H}", "side": side, "size": SIZE, "same_pixels": bool(same)}
        crop = compare("crops", {"(a) device": lambda: image_processing_batch(dev, boxes, opts, centre_crop=True),
                                 "(b) PIL + copy": lambda: torch.from_numpy(pil_route(img, boxes, opts, centre)).cuda()},
                       loops=max(2, 32 // count), extra=extra)
        pipe = FacePipeline(FixedBoxes(mtcnn, boxes), facenet, opts)

        def host_way():
            found = pipe.detector.detect(frame)
            stack = pil_route(img, found, opts, centre)
            batch = np.zeros((padded_batch(len(found)), SIZE, SIZE, 3), np.uint8)
            batch[:len(found)] = stack
            return facenet.evaluate(batch)[:len(found)]
        same_emb = np.array_equal(np.stack([e for _, e in pipe.faces(frame)]), host_way())
        photo = compare("photo -> embeddings", {"(c) FacePipeline.faces": lambda: pipe.faces(frame), "(c) PIL in the middle": host_way},
                        loops=2, extra=dict(extra, same_embeddings=bool(same_emb)))
        print(json.dumps({"faces": count, "crops_speedup": round(crop["(b) PIL + copy"] / crop["(a) device"], 2),
                          "photo_speedup": round(photo["(c) PIL in the middle"] / photo["(c) FacePipeline.faces"], 3)}), flush=True)


if __name__ == "__main__":
    main()
