"""Fingerprint of what a training step launches and computes, for before / after comparisons of engine.py and train.py.

Grouping needs the compiled library, so the host pin (tests/plan_signature.py) cannot see grouped step lists.  This builds
four trainers with fixed seeds and FACENET_AUTOTUNE=0 -- batch-90 triplet; softmax with center loss, prelogits norm, the moving
average and RMSPROP; triplet with force_segments; the margin softmax with center loss under Adam -- and prints one JSON line
each: the names of ``step_ops`` and the SHA-256 of
P, S_mean, S_var and the optimizer slots after five captured steps.  Training is bit-reproducible, so two revisions that lower
to the same launches print byte-identical output (profiles/lowering_refactor_step_compare_*.txt,
profiles/trainer_split_step_compare_*.txt)."""
import hashlib
import json
import os
import sys
from pathlib import Path

os.environ["FACENET_AUTOTUNE"] = "0"
import torch                                    # noqa: E402

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from facenet_amd.engine import Network          # noqa: E402
from facenet_amd.train import Trainer           # noqa: E402


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def run(tag, batch, classes=None, **kw):
    net = Network(embedding_size=128, nrof_classes=classes, device="cuda:0", seed=0)
    tr = Trainer(net, batch, **kw)
    g = torch.Generator().manual_seed(1234)
    x = torch.randint(0, 256, (batch, 160, 160, 3), dtype=torch.uint8, generator=g)
    labels = None
    if classes is None:
        x[2::3] = x[1::3]          # negative = positive: every triplet violates the margin, the step has a gradient
    else:
        labels = torch.randint(0, classes, (batch,), generator=g)
    tr.set_images(x, labels)
    tr.capture()
    for _ in range(5):
        tr.step()
    torch.cuda.synchronize()
    print(json.dumps({"trainer": tag, "ops": [op.name for op in tr.step_ops], "P": sha(net.P), "S_mean": sha(net.S_mean),
                      "S_var": sha(net.S_var), "slots": [sha(s) for s in tr.slots], "loss": tr.loss_value()}))
    sys.stdout.flush()


run("triplet_90", 90, loss="triplet")
run("softmax_center_rmsprop_ema", 30, classes=10, loss="softmax", center_factor=0.01, prelogits_norm_factor=5e-4,
    moving_average_decay=0.9999, optimizer="RMSPROP")
run("triplet_force_segments", 30, loss="triplet", force_segments=True)
run("softmax_margin_center_adam", 30, classes=10, loss="softmax", margin_scale=30, margin_arc=0.5, center_factor=0.01,
    optimizer="ADAM")
