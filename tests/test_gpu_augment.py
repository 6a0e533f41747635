"""fn_augment_u8 and the augmenting input pipeline on the GPU: the kernel bit-exact against the NumPy
oracle (tests/augment_oracle.py) on ragged batches, the all-keys-off case byte-equal to fn_crop_or_pad_u8, the pipeline's
batches independent of thread / process mode and of the oversize-image fallback, and both training apps fed augmented
batches from disk."""
import itertools

import numpy as np
import pytest
import torch

from facenet_amd import dataset
from facenet_amd.config import Config, load_config
from oracle import pipeline_oracle as po
from tests import augment_oracle as ao

pytestmark = pytest.mark.gpu

SIZES = [(160, 160), (250, 250), (161, 159), (100, 300), (300, 100), (1, 1), (159, 160), (165, 155), (96, 96), (182, 182),
         (183, 97), (2, 513), (95, 181)]


def _arrays(seed=3):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in SIZES]


def _draws(n, crop, flip, rotate, seed):
    return dataset.Augmentation(random_crop=crop, random_flip=flip, random_rotate=rotate, seed=seed).draw(n)


@pytest.mark.parametrize("size", [160, 96, 182])
def test_kernel_is_bit_exact_against_the_oracle(size):
    arrays = _arrays()
    hw = [a.shape[:2] for a in arrays]
    for k, (crop, flip, rotate) in enumerate(itertools.product((False, True), repeat=3)):
        params = dataset.augment_params(_draws(len(arrays), crop, flip, rotate, seed=size + k), hw, size)
        out = dataset.augment_batch(arrays, size, params)
        torch.cuda.synchronize()
        want = ao.augment_batch(arrays, size, params)
        got = out.cpu().numpy()
        bad = [i for i in range(len(arrays)) if not np.array_equal(got[i], want[i])]
        assert not bad, f"size {size} keys {(crop, flip, rotate)}: images {bad} differ ({[SIZES[i] for i in bad]})"


def test_explicit_angles_and_offsets():
    """Hand-set records: large angles, negative and positive offsets on both axes, flip with padding."""
    arrays = _arrays(5)
    rng = np.random.default_rng(9)
    n, size = len(arrays), 96
    p = np.zeros(n, dataset.AUGMENT_PARAM)
    theta = rng.uniform(-180, 180, n)
    p["cos"], p["sin"] = np.cos(np.deg2rad(theta)), np.sin(np.deg2rad(theta))
    p["y0"] = rng.integers(-40, 120, n)
    p["x0"] = rng.integers(-40, 120, n)
    p["flip"] = rng.integers(0, 2, n)
    out = dataset.augment_batch(arrays, size, p)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), ao.augment_batch(arrays, size, p))


def test_all_keys_off_equals_crop_or_pad():
    arrays = _arrays(7)
    for size in (160, 96, 182):
        params = dataset.augment_params(_draws(len(arrays), False, False, False, seed=0), [a.shape[:2] for a in arrays], size)
        got = dataset.augment_batch(arrays, size, params)
        want = dataset.crop_or_pad_batch(arrays, size)
        torch.cuda.synchronize()
        assert torch.equal(got, want)


def test_quarter_turn_is_exact():
    rng = np.random.default_rng(2)
    arrays = [rng.integers(0, 256, (n, n, 3), dtype=np.uint8) for n in (160, 96, 7)]
    p = np.zeros(3, dataset.AUGMENT_PARAM)
    p["cos"], p["sin"] = 0.0, 1.0
    p["y0"] = p["x0"] = [0, -32, -76]
    out = dataset.augment_batch(arrays, 160, p).cpu().numpy()
    assert np.array_equal(out[0], np.rot90(arrays[0], 1))
    assert np.array_equal(out[1, 32:128, 32:128], np.rot90(arrays[1], 1)) and out[1, :32].max() == 0
    assert np.array_equal(out[2, 76:83, 76:83], np.rot90(arrays[2], 1))


def test_argument_checks():
    arrays = _arrays()[:2]
    p = np.zeros(2, dataset.AUGMENT_PARAM)
    with pytest.raises(ValueError):
        dataset.augment_batch(arrays, 161, p)                       # S must be even (12-byte quads)
    with pytest.raises(ValueError):
        dataset.augment_batch(arrays, 160, p[:1])
    assert dataset.augment_batch([], 160, p[:0]).shape == (0, 160, 160, 3)


def _write_db(root, classes, per_class, sizes, seed=0):
    from PIL import Image
    rng = np.random.default_rng(seed)
    truth = {}
    for c in range(classes):
        d = root / f"id_{c:03d}"
        d.mkdir()
        for i in range(per_class):
            h, w = sizes[(c * per_class + i) % len(sizes)]
            arr = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
            f = d / f"img_{i:03d}.png"
            Image.fromarray(arr).save(f)
            truth[str(f)] = arr
    return truth


def _expected(truth, files, aug, size):
    arrays = [truth[f] for f in files]
    params = dataset.augment_params(aug.draw(len(files)), [a.shape[:2] for a in arrays], size)
    return ao.augment_batch(arrays, size, params)


def test_pipeline_modes_agree_and_follow_the_seed(tmp_path):
    truth = _write_db(tmp_path, 4, 9, [(182, 182), (250, 250), (150, 170), (480, 640), (161, 159), (1, 1)])
    db = dataset.Database(Config({"path": str(tmp_path)}))
    loader = dataset.ImageLoader(Config({"size": 160}))
    on = dict(random_crop=True, random_flip=True, random_rotate=True)

    def batches(seed, **kw):
        pipe = db.tf_dataset_api(loader, batch_size=10, augment=dataset.Augmentation(**on, seed=seed), **kw)
        out = [(x.cpu().numpy(), y.cpu().numpy()) for x, y in pipe]
        pipe.close()
        return out

    threads = batches(5, workers=4)
    assert [len(b[1]) for b in threads] == [10, 10, 10, 6]
    aug = dataset.Augmentation(**on, seed=5)
    files = db.files
    for i, (x, y) in enumerate(threads):
        assert np.array_equal(x, _expected(truth, files[10 * i:10 * i + 10], aug, 160)), f"batch {i}"
        assert np.array_equal(y, db.labels[10 * i:10 * i + 10])
    # shared-memory process mode: a 1 MiB stride holds every image; the default stride sends the 480 x 640 image through the
    # packing fallback
    for stride in (1 << 20, 300 * 300 * 3):
        procs = batches(5, workers=2, processes=True, max_image_bytes=stride)
        assert len(procs) == len(threads)
        for (a, la), (b, lb) in zip(threads, procs):
            assert np.array_equal(a, b) and np.array_equal(la, lb), f"stride {stride}"
    other = batches(6, workers=4)
    assert not np.array_equal(other[0][0], threads[0][0])
    # no augmentation: exactly the centre crop / pad, also for the batches decoded before the fallback grew the stride
    for kw in (dict(workers=4), dict(workers=2, processes=True)):
        plain = db.tf_dataset_api(loader, batch_size=10, **kw)
        got = [x.cpu().numpy() for x, _ in plain]
        plain.close()
        for i, x in enumerate(got):
            assert np.array_equal(x, np.stack([po.resize_with_crop_or_pad(truth[f], 160, 160) for f in files[10 * i:10 * i + 10]])), (kw, i)


def _record_plan(pipe, seen):
    plan = pipe._plan

    def recording():
        for files, labels in plan():
            seen.append(list(files))
            yield files, labels

    pipe._plan = recording


def _first_batch(it, keep):
    for x, y in it:
        if not keep:
            keep.append(x.clone())
        yield x, y


def test_training_apps_feed_augmented_batches(tmp_path):
    from facenet_amd.apps import train_softmax as ts, train_tripletloss as tt
    data = tmp_path / "data"
    data.mkdir()
    truth = _write_db(data, 20, 5, [(182, 182)])
    cfg = load_config(None, {"batch_size": 12, "seed": 1,
                             "image": {"size": 160, "normalization": 0, "random_crop": True, "random_flip": True, "random_rotate": True},
                             "dataset": {"path": str(data)},
                             "train": {"epoch": {"nrof_epochs": 1, "size": 2}, "learning_rate": {"schedule": [[1, 0.05]]}}})
    logs, seen, first = [], [], []
    dbase, batches = ts.dataset_batches(cfg, log=logs.append, workers=4, processes=False)
    _record_plan(batches, seen)
    net, tr = ts.train_softmax(cfg, dbase.nrof_classes, _first_batch(batches, first), embedding_size=128, log=logs.append)
    batches.close()
    assert logs[0].startswith("augmentation:") and all(k in logs[0] for k in dataset.AUGMENT_KEYS)
    assert np.isfinite(tr.loss_value())
    aug = dataset.Augmentation(random_crop=True, random_flip=True, random_rotate=True, seed=cfg.seed)
    want = _expected(truth, seen[0], aug, 160)
    assert np.array_equal(first[0].cpu().numpy(), want)
    assert not np.array_equal(want, np.stack([truth[f][11:171, 11:171] for f in seen[0]]))     # it is not the centre crop

    cfg.dataset.path = str(data)                  # Database() walks the config's path (as the reference's does)
    logs, seen, first = [], [], []
    pipe = tt.dataset_pools(cfg, log=logs.append, workers=4, processes=False)
    _record_plan(pipe, seen)
    net, tr = tt.train_tripletloss(cfg, people_per_batch=cfg.nrof_classes_per_batch, images_per_person=cfg.nrof_examples_per_class,
                                   nrof_triplets=8, pools=(x for x, _ in _first_batch(pipe, first)), log=logs.append)
    pipe.close()
    assert logs[0].startswith("augmentation:") and "triplet loss" in logs[-1] and np.isfinite(tr.loss_value())
    aug = dataset.Augmentation(random_crop=True, random_flip=True, random_rotate=True, seed=cfg.seed)
    assert np.array_equal(first[0].cpu().numpy(), _expected(truth, seen[0], aug, 160))
