"""Training-time augmentation, host side: Augmentation.from_config, the per-image draws and their
resolution into fn_augment_param records, and the NumPy oracle against its closed-form special cases.  No GPU needed."""
import numpy as np
import pytest

from facenet_amd import dataset
from facenet_amd.config import Config, load_config
from oracle import pipeline_oracle as po
from tests import augment_oracle as ao

KEYS = dataset.AUGMENT_KEYS


def test_from_config_is_none_when_every_key_is_off_or_missing():
    assert dataset.Augmentation.from_config(Config({"size": 160}), 0) is None
    assert dataset.Augmentation.from_config(load_config(None).image, 0) is None
    assert dataset.Augmentation.from_config(Config({k: False for k in KEYS}), 0) is None
    for k in KEYS:
        a = dataset.Augmentation.from_config(Config({"size": 160, k: True}), 7)
        assert a is not None and a.seed == 7 and [getattr(a, j) for j in KEYS] == [j == k for j in KEYS]
        assert k in repr(a)


def test_draws_are_reproducible_and_keys_do_not_disturb_each_other():
    on = dict(random_crop=True, random_flip=True, random_rotate=True)
    a, b = dataset.Augmentation(**on, seed=3), dataset.Augmentation(**on, seed=3)
    da = np.concatenate([a.draw(5), a.draw(11)])
    assert np.array_equal(da, b.draw(16))                           # the stream does not depend on how it is batched
    dc = dataset.Augmentation(**on, seed=4).draw(16)
    assert not np.array_equal(da["ry"], dc["ry"]) and not np.array_equal(da["theta"], dc["theta"])
    assert np.all((da["theta"] >= -10) & (da["theta"] < 10)) and np.all(da["ry"] >= 0) and np.all(da["rx"] >= 0)
    # crop and flip draws are the same whether rotation is on or off; an off key cancels only its own effect
    cf = dataset.Augmentation(random_crop=True, random_flip=True, seed=3).draw(16)
    assert np.array_equal(cf["ry"], da["ry"]) and np.array_equal(cf["rx"], da["rx"]) and np.array_equal(cf["flip"], da["flip"])
    assert np.all(cf["theta"] == 0)
    r = dataset.Augmentation(random_rotate=True, seed=3).draw(16)
    assert np.array_equal(r["theta"], da["theta"]) and np.all(r["ry"] == -1) and np.all(r["rx"] == -1) and not r["flip"].any()


@pytest.mark.parametrize("h", [100, 159, 160, 161, 182, 250])
def test_offsets_stay_in_range(h):
    size, n = 160, 400
    a = dataset.Augmentation(random_crop=True, seed=h)
    hw = np.tile([h, h + 3], (n, 1))
    p = dataset.augment_params(a.draw(n), hw, size)
    for field, ext in (("y0", h), ("x0", h + 3)):
        if ext <= size:
            assert np.all(p[field] == -((size - ext) // 2))                  # centred zero padding, as today
        else:
            assert p[field].min() >= 0 and p[field].max() <= ext - size
            if ext - size >= 2:
                assert len(np.unique(p[field])) > 1
    centre = dataset.augment_params(dataset.Augmentation(random_flip=True, seed=0).draw(n), hw, size)
    want = [(h - size) // 2 if h > size else -((size - h) // 2), (h + 3 - size) // 2 if h + 3 > size else -((size - h - 3) // 2)]
    assert np.all(centre["y0"] == want[0]) and np.all(centre["x0"] == want[1])
    assert np.all(centre["cos"] == 1) and np.all(centre["sin"] == 0)


def test_half_of_the_images_are_flipped():
    n = 20000
    flips = int(dataset.Augmentation(random_flip=True, seed=11).draw(n)["flip"].sum())
    assert abs(flips - n / 2) <= 4 * np.sqrt(n / 4)                 # 4 sigma of Binomial(n, 1/2)


def test_rotation_params_are_float32_of_float64_trig():
    d = dataset.Augmentation(random_rotate=True, seed=5).draw(64)
    p = dataset.augment_params(d, np.tile([182, 182], (64, 1)), 160)
    rad = np.deg2rad(d["theta"])
    assert np.array_equal(p["cos"], np.cos(rad).astype(np.float32)) and np.array_equal(p["sin"], np.sin(rad).astype(np.float32))
    assert np.all(p["y0"] == 11) and np.all(p["x0"] == 11)


def test_param_record_matches_the_c_struct():
    assert dataset.AUGMENT_PARAM.itemsize == 20
    assert [dataset.AUGMENT_PARAM.fields[k][1] for k in ("y0", "x0", "flip", "cos", "sin")] == [0, 4, 8, 12, 16]


@pytest.mark.parametrize("shape", [(160, 160), (182, 182), (100, 300), (1, 1), (161, 159), (250, 170)])
def test_oracle_identity_is_crop_or_pad(shape):
    img = np.random.default_rng(0).integers(0, 256, shape + (3,), dtype=np.uint8)
    p = dataset.augment_params(_centre(), [shape], 160)[0]
    assert np.array_equal(ao.augment(img, 160, p["y0"], p["x0"], False, p["cos"], p["sin"]), po.resize_with_crop_or_pad(img, 160, 160))
    # the resampling path at angle zero is the identity too
    assert np.array_equal(ao.rotate(img, 1.0, 0.0), img)


def _centre():
    d = np.zeros(1, dataset.AUGMENT_DRAW)
    d["ry"] = d["rx"] = -1
    return d


def test_oracle_quarter_turn_and_flip():
    for n in (7, 8, 160):
        img = np.random.default_rng(n).integers(0, 256, (n, n, 3), dtype=np.uint8)
        assert np.array_equal(ao.rotate(img, 0.0, 1.0), np.rot90(img, 1))             # counter-clockwise as displayed
        assert np.array_equal(ao.augment(img, n, 0, 0, True, 1.0, 0.0), img[:, ::-1])
    img = np.random.default_rng(1).integers(0, 256, (9, 13, 3), dtype=np.uint8)
    assert np.array_equal(ao.crop_or_pad(img, 8, 1, 2), img[1:9, 2:10])
    assert np.array_equal(ao.crop_or_pad(img, 16, -3, -1)[3:12, 1:14], img)


def test_oracle_rotation_is_bilinear_with_zero_fill():
    img = np.full((40, 40, 3), 200, np.uint8)
    c, s = np.float32(np.cos(np.deg2rad(10.0))), np.float32(np.sin(np.deg2rad(10.0)))
    r = ao.rotate(img, c, s)
    assert np.all(r[18:22, 18:22] == 200)                                             # the interior keeps its value
    assert r[0, 0].max() == 0 and r[0, 39].max() == 0                                 # corners rotate in from outside
