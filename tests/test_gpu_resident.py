"""The resident input pipeline on the GPU: fn_resident_batch_u8 bit-exact against the NumPy oracle
(tests/augment_oracle.py), against fn_augment_u8 on the same images packed batch-locally and, without records, against
fn_crop_or_pad_u8; byte offsets past 2^31; rows outside the store; the refused arguments; ResidentPipeline against BatchPipeline
batch for batch; and both training apps trained from the store and from the files to the same loss, bit for bit."""
import functools
import itertools
import random
import re

import numpy as np
import pytest
import torch

from facenet_amd import dataset, resident
from facenet_amd._lib import FacenetHipError
from facenet_amd.config import Config, load_config
from tests import augment_oracle as ao
from tests.test_gpu_augment import _expected, _first_batch, _record_plan, _write_db

pytestmark = pytest.mark.gpu

SIZES = [(182, 182), (250, 250), (150, 170), (161, 159), (17, 5), (1, 1)]
ROWS = np.array([3, 0, 5, 2, 1, 2, 4], np.int32)          # not monotone; row 0, row M - 1, and row 2 twice
ON = dict(random_crop=True, random_flip=True, random_rotate=True)


@functools.lru_cache(maxsize=None)
def _arrays():
    rng = np.random.default_rng(11)
    return tuple(rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in SIZES)


@functools.lru_cache(maxsize=None)
def _cases(size):
    """(name, records for ROWS, oracle output) for every key combination and one hand-set case; computed once per size."""
    arrays = [_arrays()[r] for r in ROWS]
    hw = [a.shape[:2] for a in arrays]
    out = []
    for k, (crop, flip, rotate) in enumerate(itertools.product((False, True), repeat=3)):
        draws = dataset.Augmentation(random_crop=crop, random_flip=flip, random_rotate=rotate, seed=size + k).draw(len(ROWS))
        out.append([f"keys {(crop, flip, rotate)}", dataset.augment_params(draws, hw, size)])
    rng = np.random.default_rng(size)
    p = np.zeros(len(ROWS), dataset.AUGMENT_PARAM)
    theta = rng.uniform(-180, 180, len(ROWS))
    p["cos"], p["sin"] = np.cos(np.deg2rad(theta)), np.sin(np.deg2rad(theta))
    p["y0"], p["x0"], p["flip"] = rng.integers(-40, 120, len(ROWS)), rng.integers(-40, 120, len(ROWS)), rng.integers(0, 2, len(ROWS))
    out.append(["hand-set", p])
    for case in out:
        case.append(ao.augment_batch(arrays, size, case[1]))
    return out


def _store(align=16):
    arrays = list(_arrays())
    return resident.ResidentDataset.from_arrays(arrays, [f"img{i}" for i in range(len(arrays))], np.arange(len(arrays)), align=align)


@pytest.mark.parametrize("align", [16, 1])
@pytest.mark.parametrize("size", [160, 96])
def test_batch_is_bit_exact(size, align):
    store = _store(align)
    if align == 1:
        assert any(o % 2 for o in store.host_offsets.tolist())                 # odd byte offsets are really exercised
    else:
        assert not any(o % 16 for o in store.host_offsets.tolist())
    assert store.nrof_images == len(SIZES) and "6 images" in repr(store)
    for i, a in enumerate(_arrays()):
        assert np.array_equal(store.image(i), a)
    local = [_arrays()[r] for r in ROWS]
    twice = np.flatnonzero(ROWS == 2)
    for name, params, want in _cases(size):
        if name in ("hand-set", "keys (True, True, True)"):
            assert params[twice[0]] != params[twice[1]], "the row taken twice must get two different records"
        got = store.batch(ROWS, size, params)
        other = dataset.augment_batch(local, size, params)                      # the same images, packed batch-locally
        torch.cuda.synchronize()
        bad = [n for n in range(len(ROWS)) if not np.array_equal(got[n].cpu().numpy(), want[n])]
        assert not bad, f"size {size} align {align} {name}: batch images {bad} (rows {ROWS[bad]}) differ from the oracle"
        assert torch.equal(got, other), f"size {size} align {align} {name}: differs from fn_augment_u8"
        one = store.batch(ROWS[5:6], size, params[5:6])                         # N = 1
        assert one.shape == (1, size, size, 3) and torch.equal(one[0], got[5])
    plain = store.batch(ROWS, size)
    want = dataset.crop_or_pad_batch(local, size)
    torch.cuda.synchronize()
    assert torch.equal(plain, want), "params = NULL differs from fn_crop_or_pad_u8"
    assert torch.equal(store.batch([4], size)[0], want[6])
    # device tensors for rows and records, and a caller's output buffer
    name, params, want = _cases(size)[-1]
    out = torch.empty(len(ROWS), size, size, 3, dtype=torch.uint8, device="cuda")
    ret = store.batch(torch.from_numpy(ROWS).cuda(), size, torch.from_numpy(params.view(np.uint8)).cuda(), out=out)
    assert ret is out and np.array_equal(out.cpu().numpy(), want)
    assert store.batch([], size).shape == (0, size, size, 3)
    with pytest.raises(ValueError):
        store.batch(ROWS, size, params[:3])


def test_byte_offsets_past_two_to_the_31():
    far = 2 ** 31 + 5
    pool = torch.empty(2 ** 31 + 2 ** 20, dtype=torch.uint8, device="cuda")     # an allocation, not a fill
    rng = np.random.default_rng(4)
    a, b = (rng.integers(0, 256, (33, 35, 3), dtype=np.uint8) for _ in range(2))
    pool[:a.size].copy_(torch.from_numpy(a.reshape(-1)))
    pool[far:far + b.size].copy_(torch.from_numpy(b.reshape(-1)))
    store = resident.ResidentDataset(pool, np.array([0, far], np.int64), np.array([[33, 35], [33, 35]], np.int32), ["a", "b"], [0, 1], "cuda")
    assert np.array_equal(store.image(1), b)
    rows = np.array([1, 0, 1], np.int32)
    got = store.batch(rows, 40).cpu().numpy()                                   # padded on both axes: the whole image comes back
    for n, src in enumerate((b, a, b)):
        assert np.array_equal(got[n, 3:36, 2:37], src) and got[n].sum() == src.sum()
    p = np.zeros(3, dataset.AUGMENT_PARAM)
    p["cos"], p["sin"], p["y0"], p["x0"], p["flip"] = np.cos(0.3), np.sin(0.3), [-3, 2, 0], [-2, -1, 4], [0, 1, 1]
    got = store.batch(rows, 32, p).cpu().numpy()
    assert np.array_equal(got, ao.augment_batch([b, a, b], 32, p))
    del store, pool
    torch.cuda.empty_cache()


def test_rows_outside_the_store_give_zero_images():
    store = _store()
    m, size = store.nrof_images, 96
    rows = np.array([-1, 2, m, 0, 2 ** 31 - 1, -2 ** 31], np.int32)
    name, params, _ = _cases(size)[-1]
    for prm in (params[:6], None):
        out = torch.full((6, size, size, 3), 255, dtype=torch.uint8, device="cuda")
        store.batch(rows, size, prm, out=out)
        good = store.batch(rows[[1, 3]], size, None if prm is None else prm[[1, 3]])
        torch.cuda.synchronize()
        assert all(int(out[n].max()) == 0 for n in (0, 2, 4, 5)), "a row outside [0, M) must give an all-zero image"
        assert torch.equal(out[[1, 3]], good) and int(good.max()) > 0


def test_argument_checks():
    store = _store()
    rows = torch.zeros(4, dtype=torch.int32, device="cuda")
    prm = torch.zeros(4 * 20, dtype=torch.uint8, device="cuda")
    out = torch.empty(4, 96, 96, 3, dtype=torch.uint8, device="cuda")
    good = dict(pool=store.pool.data_ptr(), offsets=store.offsets.data_ptr(), hw=store.hw.data_ptr(), m=store.nrof_images,
                rows=rows.data_ptr(), params=prm.data_ptr(), dst=out.data_ptr(), n=4, size=96)
    resident.resident_batch_u8(**good)
    resident.resident_batch_u8(**{**good, "params": 0})                         # NULL records are the centre crop, not an error
    for bad in (dict(pool=0), dict(offsets=0), dict(hw=0), dict(rows=0), dict(dst=0), dict(n=0), dict(n=-1), dict(n=65536), dict(size=95),
                dict(size=0), dict(m=0), dict(m=-5)):
        with pytest.raises(FacenetHipError, match="resident_batch: bad arguments"):
            resident.resident_batch_u8(**{**good, **bad})
    torch.cuda.synchronize()
    with pytest.raises(KeyError, match="nowhere.png"):
        store.rows_of(["img1", "nowhere.png", "also-missing.png"])
    assert store.rows_of(["img5", "img0"]).tolist() == [5, 0]


# ---- the pipelines on a data set from disk ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def disk(tmp_path_factory):
    """20 classes x 5 PNG files (lossless) with ragged sizes, their pixels, the Database and its resident store."""
    root = tmp_path_factory.mktemp("resident") / "data"
    root.mkdir()
    truth = _write_db(root, 20, 5, [(182, 182), (250, 250), (150, 170), (161, 159), (17, 5), (1, 1)])
    db = dataset.Database(Config({"path": str(root)}))
    store = resident.ResidentDataset.from_database(db, workers=4)
    return root, truth, db, store


def test_store_from_database_and_from_a_cache_hold_the_same_images(disk, tmp_path):
    root, truth, db, store = disk
    assert store.files == db.files and np.array_equal(store.labels.cpu().numpy(), db.labels) and store.info["cache"] == "none"
    cached = resident.ResidentDataset.from_database(db, cache=tmp_path / "pack", workers=4)
    again = resident.ResidentDataset.from_database(db, cache=tmp_path / "pack", workers=4)
    assert (cached.info["cache"], again.info["cache"]) == ("miss", "hit")
    assert again.files == db.files and torch.equal(again.pool, cached.pool) and torch.equal(again.pool, store.pool)
    assert torch.equal(again.offsets, store.offsets) and torch.equal(again.hw, store.hw)
    for i in (0, 7, 99):
        assert np.array_equal(again.image(i), truth[db.files[i]])
    bare = resident.ResidentDataset.from_pack(tmp_path / "pack")
    assert bare.files[0] == "id_000/img_000.png" and bare.nbytes == store.nbytes


def _seed(seed, augmented):
    random.seed(seed)
    np.random.seed(seed)
    return dataset.Augmentation(**ON, seed=seed) if augmented else None


def _take(pipe, count):
    out = []
    for x, y in pipe:
        out.append((x.cpu().numpy(), y.cpu().numpy()))
        if len(out) == count:
            break
    pipe.close()
    return out


@pytest.mark.parametrize("augmented", [True, False])
def test_pipelines_agree(disk, augmented):
    root, truth, db, store = disk
    loader = dataset.ImageLoader(Config({"size": 160}))
    files, labels = db.files[:72:2][::-1], db.labels[:72:2][::-1]                # 36 images in an order of their own
    assert len(files) == 36

    def both(make, count, seed=5):
        out = []
        for kw in (dict(workers=4), dict(resident=store)):
            aug = _seed(seed, augmented)
            out.append(_take(make(aug, kw), count))
        assert isinstance(make(None, dict(resident=store)), dataset.ResidentPipeline)
        return out

    # a finite epoch of 36 images at batch 10: the short last batch of 6
    epoch = lambda aug, kw: dataset.tf_dataset_api(files, labels, loader, 10, augment=aug, **kw)
    a, b = both(epoch, None)
    assert [len(y) for _, y in b] == [10, 10, 10, 6] and len(epoch(None, dict(resident=store))) == 4
    aug = dataset.Augmentation(**ON, seed=5)
    for i, ((xa, ya), (xb, yb)) in enumerate(zip(a, b)):
        assert np.array_equal(xa, xb) and np.array_equal(ya, yb) and yb.dtype == np.int64, f"epoch batch {i}"
        assert np.array_equal(yb, labels[10 * i:10 * i + 10])
        if augmented:
            assert np.array_equal(xb, _expected(truth, files[10 * i:10 * i + 10], aug, 160))
    # a shuffled repeating stream (processes / workers are ignored with a store)
    stream = lambda aug, kw: db.tf_dataset_api(loader, 12, buffer_size=10, repeat=True, augment=aug, **{"processes": False, **kw})
    a, b = both(stream, 5)
    assert len(b) == 5 and stream(None, dict(resident=store)).cardinality() is None
    for i, ((xa, ya), (xb, yb)) in enumerate(zip(a, b)):
        assert np.array_equal(xa, xb) and np.array_equal(ya, yb), f"stream batch {i}"
    # P x K batches
    equal = lambda aug, kw: dataset.pipeline_with_equal_batches(loader, db.classes, Config({}), augment=aug, **kw)
    a, c = both(equal, 3)
    for i, ((xa, ya), (xb, yb)) in enumerate(zip(a, c)):
        assert xb.shape == (100, 160, 160, 3) and np.array_equal(xa, xb) and np.array_equal(ya, yb), f"P x K batch {i}"
    # another seed: other batches
    other = both(stream, 1, seed=6)[1]
    assert not np.array_equal(other[0][0], b[0][0])


def test_unknown_file_raises_before_anything_is_launched(disk, monkeypatch):
    root, truth, db, store = disk
    launched = []
    monkeypatch.setattr(store, "launch", lambda *a, **k: launched.append(a))
    loader = dataset.ImageLoader(Config({"size": 160}))
    files = db.files[:5] + [str(root / "id_000" / "not-there.png")] + db.files[5:9]
    pipe = dataset.tf_dataset_api(files, list(range(10)), loader, 10, resident=store)
    with pytest.raises(KeyError, match="not-there.png"):
        next(iter(pipe))
    assert not launched


def _config(root, **dataset_keys):
    return load_config(None, {"batch_size": 12, "seed": 1, "image": {"size": 160, "normalization": 0, **ON},
                              "dataset": {"path": str(root), **dataset_keys},
                              "train": {"epoch": {"nrof_epochs": 1, "size": 2}, "learning_rate": {"schedule": [[1, 0.05]]}}})


def _bits(x: float) -> bytes:
    return np.float64(x).tobytes()


def test_softmax_app_trains_the_same_from_the_store(disk, tmp_path):
    from facenet_amd.apps import train_softmax as ts
    root, truth, db, _ = disk
    runs = {}
    for name, keys in (("resident", dict(resident=True, resident_cache=str(tmp_path / "pack"))), ("files", {})):
        cfg = _config(root, **keys)
        logs, seen, first = [], [], []
        random.seed(3)
        dbase, batches = ts.dataset_batches(cfg, log=logs.append, workers=4, processes=False)
        assert isinstance(batches, dataset.ResidentPipeline if keys else dataset.BatchPipeline)
        _record_plan(batches, seen)
        net, tr = ts.train_softmax(cfg, dbase.nrof_classes, _first_batch(batches, first), embedding_size=128, log=logs.append)
        batches.close()
        aug = dataset.Augmentation(**ON, seed=cfg.seed)
        assert np.array_equal(first[0].cpu().numpy(), _expected(truth, seen[0], aug, 160)), name
        runs[name] = (tr.loss_value(), logs, seen)
    assert np.isfinite(runs["files"][0]) and _bits(runs["resident"][0]) == _bits(runs["files"][0])
    assert runs["resident"][2] == runs["files"][2]
    lines = [l for l in runs["resident"][1] if l.startswith("resident data set:")]
    assert len(lines) == 1 and "100 images" in lines[0] and "GiB" in lines[0] and "cache miss" in lines[0]
    assert runs["resident"][1].index(lines[0]) == 1 and runs["resident"][1][0].startswith("augmentation:")
    assert not [l for l in runs["files"][1] if "resident" in l]
    assert [l for l in runs["resident"][1] if l != lines[0]][:1] == runs["files"][1][:1]


def test_triplet_app_trains_the_same_from_the_store(disk):
    from facenet_amd.apps import train_tripletloss as tt
    root, truth, db, _ = disk
    runs = {}
    for name, keys in (("resident", dict(resident=True)), ("files", {})):
        cfg = _config(root, **keys)
        logs, seen, first = [], [], []
        random.seed(3)
        np.random.seed(3)
        pipe = tt.dataset_pools(cfg, log=logs.append, workers=4, processes=False)
        assert isinstance(pipe, dataset.ResidentPipeline if keys else dataset.BatchPipeline)
        _record_plan(pipe, seen)
        net, tr = tt.train_tripletloss(cfg, people_per_batch=cfg.nrof_classes_per_batch, images_per_person=cfg.nrof_examples_per_class,
                                       nrof_triplets=8, pools=(x for x, _ in _first_batch(pipe, first)), log=logs.append)
        pipe.close()
        aug = dataset.Augmentation(**ON, seed=cfg.seed)
        assert np.array_equal(first[0].cpu().numpy(), _expected(truth, seen[0], aug, 160)), name
        runs[name] = (tr.loss_value(), logs, seen)
    assert np.isfinite(runs["files"][0]) and _bits(runs["resident"][0]) == _bits(runs["files"][0])
    assert runs["resident"][2] == runs["files"][2]
    lines = [l for l in runs["resident"][1] if l.startswith("resident data set:")]
    assert len(lines) == 1 and "no cache" in lines[0] and runs["resident"][1].index(lines[0]) == 1
    assert not [l for l in runs["files"][1] if "resident" in l]


def test_cap_is_an_error_that_names_both_byte_counts(disk):
    from facenet_amd.apps import train_softmax as ts, train_tripletloss as tt
    root, truth, db, store = disk
    for build in (lambda cfg: ts.dataset_batches(cfg, log=lambda s: None), lambda cfg: tt.dataset_pools(cfg, log=lambda s: None)):
        with pytest.raises(ValueError) as err:
            build(_config(root, resident=True, resident_bytes=1000))
        found = re.search(r"needs (\d+) bytes.* (\d+) bytes are allowed", str(err.value))
        assert found and int(found.group(1)) == store.nbytes and int(found.group(2)) == 1000
    with pytest.raises(ValueError, match="1000 bytes are allowed"):
        resident.ResidentDataset.from_arrays(list(_arrays()), list("abcdef"), range(6), max_bytes=1000)
    assert resident.default_max_bytes("cuda") == torch.cuda.mem_get_info()[1] // 2
