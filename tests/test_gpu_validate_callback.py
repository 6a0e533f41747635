"""Validation inside training on the GPU (facenet_amd.callbacks): the callback inside both training apps
with the captured graph on, its embeddings against Trainer.evaluate and against the checkpoint the app wrote, training left
bit for bit as it is without validation, two data-parallel ranks, and the validate app end to end."""
import os
import socket

import numpy as np
import pytest
import torch

from facenet_amd import callbacks
from facenet_amd.config import Config, load_config
from tests.util_data import structured_images

pytestmark = pytest.mark.gpu

NCLS, BATCH = 19, 8
VALIDATE = {"every_n_epochs": 2, "validate": {"metric": 0, "nrof_folds": 3, "far_target": 1e-3}}


@pytest.fixture(autouse=True)
def _heuristic_tiles(monkeypatch):
    # trainers and models that are compared bit for bit run on the library's deterministic tile heuristic
    monkeypatch.setenv("FACENET_AUTOTUNE", "0")


def _validation_set(n=20, classes=4, seed=71):
    """Batches of 8, 8 and 4 images; every class has n / classes rows."""
    x = torch.from_numpy(structured_images(n, seed=seed))
    y = np.arange(n) % classes
    return [(x[i:i + BATCH], y[i:i + BATCH]) for i in range(0, n, BATCH)]


class _Recording(callbacks.ValidateCallback):
    """Keeps, per pass, the embeddings the statistic saw and Trainer.evaluate on the same batches right after it."""

    def validate(self, epoch1):
        report = super().validate(epoch1)
        tr = self.model.trainer
        direct = torch.cat([tr.evaluate(x, averaged=self.averaged) for x, _ in self.dataset]).cpu().numpy()
        self.passes.append((self.embeddings.copy(), direct))
        return report


def _callback(cfg, data, averaged=False, log=lambda *_: None):
    cb = _Recording(None, data, cfg.validate.every_n_epochs, cfg.train.epoch.nrof_epochs, cfg.validate, averaged=averaged, log=log)
    cb.passes = []
    return cb


def _state(net, tr):
    out = [net.P, net.S_mean, net.S_var] + list(tr.slots) + ([] if tr.shadow is None else [tr.shadow])
    return [t.clone() for t in out], tr.iterations


def _softmax(tmp_path, name, validation, decay=0.9999):
    from facenet_amd.apps.train_softmax import train_softmax
    train = {"epoch": {"nrof_epochs": 3, "size": 2}, "learning_rate": {"value": 0.01}}
    if decay is not None:
        train["moving_average_decay"] = decay
    cfg = load_config(overrides={"batch_size": 6, "train": train, "model": {"path": str(tmp_path / name)}, "validate": VALIDATE})
    x = torch.from_numpy(structured_images(6, seed=21))
    y = torch.from_numpy(np.random.default_rng(21).integers(0, NCLS, 6))
    logs = []
    cb = validation(cfg, logs) if validation else None
    net, tr = train_softmax(cfg, NCLS, batches=((x, y) for _ in iter(int, 1)), embedding_size=128, log=logs.append, validation=cb)
    torch.cuda.synchronize()
    return net, tr, cb, logs


def _check_passes(cb, report_file, moved=True):
    assert [h[0] for h in cb.history] == [2, 3] and len(cb.passes) == 2
    for seen, direct in cb.passes:
        assert seen.shape == (20, 128) and np.array_equal(seen, direct)
        np.testing.assert_allclose(np.linalg.norm(seen, axis=1), 1.0, atol=1e-5)
    if moved:                                                             # the weights changed in between
        assert not np.array_equal(cb.passes[0][0], cb.passes[1][0])
    for _, d, t_embed, t_stat in cb.history:
        assert set(d) == {"MaximumAccuracy", "FalseAlarmRate(FAR = 0.001)"} and t_embed > 0 and t_stat > 0
    text = report_file.read_text()
    assert text.count("FaceToFaceValidation ") == 2 and text.count("Area under curve (AUC)") == 4 and text.count(64 * "-") == 2
    assert cb._resident is not None and all(x.is_cuda for x, _ in cb._resident)      # decoded once, kept on the device
    print("validation passes (epoch, s embedding, s statistics):", [(h[0], round(h[2], 4), round(h[3], 4)) for h in cb.history])


def test_softmax_training_with_validation(tmp_path):
    from facenet_amd.api import FaceNet
    data = _validation_set()
    plain_net, plain_tr, _, plain_logs = _softmax(tmp_path, "plain", None)
    want, want_t = _state(plain_net, plain_tr)
    for averaged in (False, True):
        name = "averaged_run" if averaged else "raw_run"
        net, tr, cb, logs = _softmax(tmp_path, name, lambda cfg, logs: _callback(cfg, data, averaged, logs.append))
        got, got_t = _state(net, tr)
        assert got_t == want_t == 6 and len(got) == len(want)
        for a, b in zip(got, want):
            assert torch.equal(a, b)                                      # training is what it is without validation
        _check_passes(cb, tmp_path / name / "report.txt")
        assert [l for l in logs if l.startswith("epoch ")] and len([l for l in logs if l.startswith("epoch ")]) == len(plain_logs) == 3
        assert "perform validation for epoch 2" in logs and "perform validation for epoch 3" in logs
        # after the last epoch the callback saw the model the app wrote
        path = tmp_path / name / ("averaged" if averaged else f"{name}.npz")
        model = FaceNet(Config({"path": str(path), "embedding_size": 128, "normalize": True}))
        saved = np.concatenate([model.evaluate(x) for x, _ in data])
        assert np.array_equal(saved, cb.passes[-1][0])
    assert not (tmp_path / "plain" / "report.txt").exists()


def test_averaged_validation_needs_the_moving_average(tmp_path):
    with pytest.raises(ValueError, match="moving_average_decay"):
        _softmax(tmp_path, "none", lambda cfg, logs: _callback(cfg, _validation_set(), True), decay=None)


def test_triplet_training_with_validation(tmp_path):
    from facenet_amd.apps.train_tripletloss import train_tripletloss
    data = _validation_set()
    states = []
    for validate in (False, True):
        name = "with" if validate else "without"
        train = {"epoch": {"nrof_epochs": 3, "size": 2}, "learning_rate": {"value": 0.01}}
        cfg = load_config(overrides={"train": train, "model": {"path": str(tmp_path / name)}, "validate": VALIDATE})
        cb = _callback(cfg, data) if validate else None
        g = torch.Generator().manual_seed(3)
        pools = (torch.randint(0, 256, (12, 160, 160, 3), dtype=torch.uint8, generator=g) for _ in iter(int, 1))
        logs = []
        net, tr = train_tripletloss(cfg, people_per_batch=6, images_per_person=2, nrof_triplets=4, pools=pools, log=logs.append, validation=cb)
        torch.cuda.synchronize()
        states.append(_state(net, tr))
        assert len([l for l in logs if "triplet loss" in l]) == 3
    (without, t0), (with_, t1) = states
    assert t0 == t1 == 6
    for a, b in zip(with_, without):
        assert torch.equal(a, b)
    _check_passes(cb, tmp_path / "with" / "report.txt", moved=False)     # random pools may select no violating triplet


# ---- data parallelism ------------------------------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _dp_set():
    x = torch.from_numpy(structured_images(36, seed=72))           # 5 batches, the last one short: not a multiple of batch x world
    y = np.arange(36) % 5
    return [(x[i:i + BATCH], y[i:i + BATCH]) for i in range(0, 36, BATCH)]


def _embed(rank, world, pg):
    from facenet_amd.engine import Network
    from facenet_amd.train import Trainer
    net = Network(embedding_size=128, device="cuda:0", nrof_classes=NCLS, train_dtype=torch.float16, seed=0)
    tr = Trainer(net, batch=4, loss="softmax", lr=0.01, world_size=world, process_group=pg)
    cb = callbacks.ValidateCallback(None, _dp_set(), 1, 1, Config({"validate": VALIDATE["validate"]}), log=lambda *_: None)
    cb.attach(tr, rank=rank, world=world, process_group=pg)
    emb, labels = cb.embed()
    report = cb.on_epoch_end(0)
    return emb, labels, report, cb


def _rank(rank, world, port, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["FACENET_AUTOTUNE"] = "0"
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        emb, labels, report, cb = _embed(rank, world, dist.group.WORLD)
        q.put((rank, emb, labels, report is not None, len(cb.history), len(cb._resident)))
    finally:
        dist.destroy_process_group()


def test_two_ranks_gather_the_embeddings_in_order():
    import torch.multiprocessing as mp
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_rank, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=600) for _ in range(world)], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    single, labels, report, cb = _embed(0, 1, None)
    assert single.shape == (36, 128) and report is not None
    for rank, emb, lab, reported, n_history, n_resident in res:
        assert np.array_equal(emb, single) and np.array_equal(lab, labels)       # every rank holds the gathered set, in order
        assert reported == (rank == 0) and n_history == (1 if rank == 0 else 0)  # rank 0 computes and reports
        assert n_resident == len(callbacks.shard(5, rank, world))                 # each rank keeps its own batches only


# ---- the validate app ------------------------------------------------------------------------------------------------------------
def test_validate_app_end_to_end(tmp_path):
    from PIL import Image
    from facenet_amd import dataset
    from facenet_amd.api import FaceNet
    from facenet_amd.apps.validate import load_options, validate
    from facenet_amd.facenet import evaluate_embeddings
    from facenet_amd.statistics import FaceToFaceValidation
    rng = np.random.default_rng(0)
    data = tmp_path / "faces"
    data.mkdir()
    # two classes: every table entry is the sum of at most two workgroups' contributions, so the tables (and with them the
    # thresholds picked on plateaus of the accuracy) do not depend on the order of the fp64 atomics
    for c, n in enumerate((7, 8)):
        (data / f"id_{c:03d}").mkdir()
        for i in range(n):
            Image.fromarray(rng.integers(0, 256, (160, 160, 3), dtype=np.uint8)).save(data / f"id_{c:03d}" / f"img_{i:03d}.png")
    model_dir = tmp_path / "model"
    model_dir.mkdir()
    overrides = {"batch_size": 8, "dataset": {"path": str(data)}, "model": {"path": None, "embedding_size": 128},
                 "validate": {"nrof_folds": 3, "metric": 1}, "file": str(model_dir / "report.txt")}
    lines = []
    report = validate(load_options(overrides=overrides), log=lambda s: lines.append(str(s)))
    text = (model_dir / "report.txt").read_text().split("\n")
    assert text[0] == 64 * "-" and text[1] == "Database" and text[2] == str(data)
    assert "Number of classes 2 " in text and "Number of images 15" in text
    at = text.index("EvaluationOfEmbeddings")
    assert text[at - 1] == 64 * "-" and text[at + 1].startswith("model: path: ") and text[at + 3] == "embedding size: (15, 128)"
    assert text[at + 4] == 64 * "-" and text[at + 5].startswith("FaceToFaceValidation 20") and text[at + 6] == "metric: 1"
    assert "MaximumAccuracy" in text and "FalseAlarmRate(FAR = 0.001)" in text and text[-2].startswith("elapsed time: ") and text[-1] == ""
    assert any(l.startswith("Report has been written to the file") for l in lines)
    # the same by hand
    opt = load_options(overrides=overrides)
    dbase = dataset.Database(opt.dataset)
    model_cfg = Config(opt.model.as_dict)
    model_cfg.image = opt.image
    facenet = FaceNet(model_cfg)
    batches = dbase.tf_dataset_api(loader=dataset.ImageLoader(config=opt.image), batch_size=8)
    emb, labels = evaluate_embeddings(facenet.evaluate, ((x, l.cpu()) for x, l in batches))
    np.testing.assert_allclose(np.linalg.norm(emb, axis=1), 1.0, atol=1e-5)                   # normalize was forced on
    by_hand = FaceToFaceValidation(emb, labels, opt.validate)
    for crit, d in by_hand.dict.items():
        for key, val in d.items():
            assert report.dict[crit][key] == val, (crit, key)
