"""The moving average of the weights on the host: the fp32 oracle against a float64 closed form, the fp32
switch point of the decay ramp, the checkpoint names of the shadow variables and the config helper of the training apps."""
import numpy as np
import pytest

from facenet_amd import keras_names
from facenet_amd.config import Config, load_config
from facenet_amd.train import check_moving_average_decay, moving_average_decay
from tests import ema_oracle as eo


def test_oracle_matches_the_float64_closed_form_for_small_t():
    # from s_0 = w_0 with w fixed after the first step: s_t - w = (s_0 - w) * prod_{k<=t} d_k, d_k = (1 + k) / (10 + k) early on
    rng = np.random.default_rng(0)
    s0 = rng.standard_normal(1000).astype(np.float32)
    w = rng.standard_normal(1000).astype(np.float32)
    s = s0.copy()
    prod = 1.0
    for t in range(1, 9):
        s = eo.update(s, w, t, 0.9999)
        prod *= (1.0 + t) / (10.0 + t)
        want = w.astype(np.float64) + (s0.astype(np.float64) - w) * prod
        assert s.dtype == np.float32
        assert np.abs(s - want).max() <= 8 * t * np.spacing(np.float32(np.abs(want).max()))
    # one step is exactly three rounded fp32 operations with d = 2/11 at t = 1
    one_minus_d = np.float32(1.0) - np.float32(np.float32(2.0) / np.float32(11.0))
    assert np.array_equal(eo.update(s0, w, 1, 0.9999), s0 - (s0 - w) * one_minus_d)
    # a small decay caps the ramp from the start
    assert eo.decay_at(1, 0.1) == np.float32(0.1)


def test_switch_point_of_the_decay_in_fp32():
    t = eo.switch_point(0.9999)
    d = np.float32(0.9999)
    ramp = lambda k: np.float32(np.float32(1 + k) / np.float32(10 + k))
    assert ramp(t - 1) < d <= ramp(t)
    assert eo.decay_at(t - 1, 0.9999) == ramp(t - 1) < d
    assert eo.decay_at(t, 0.9999) == d == eo.decay_at(10 ** 6, 0.9999)
    assert abs(t - 89_990) <= 50            # the real-number crossing: (1 + t) / (10 + t) = 0.9999 at t = 89 990


def test_shadow_variable_names():
    assert keras_names.moving_average_name("inception_resnet_v1/conv2d/Conv2d_1a_3x3/kernel:0") == \
        "inception_resnet_v1/conv2d/Conv2d_1a_3x3/kernel/ExponentialMovingAverage:0"
    assert keras_names.moving_average_name("InceptionResnetV2/Conv2d_1a_3x3/weights") == \
        "InceptionResnetV2/Conv2d_1a_3x3/weights/ExponentialMovingAverage:0"
    # shadows sit next to the Adam slots, and no shadow name is a model variable name
    from facenet_amd.engine import Network
    net = Network(embedding_size=128, allocate=False)
    table = net.variable_table()
    names = {k for k, _ in table}
    shadows = {keras_names.moving_average_name(k) for k, i in table if not i.endswith(("moving_mean", "moving_variance"))}
    assert not names & shadows and len(shadows) == len(table) - 2 * sum(L.has_bn for L in net.layers.values())


def test_config_helper():
    assert moving_average_decay(load_config()) is None                               # the key is not among the defaults
    for value in (None, 0, 0.0):
        assert moving_average_decay(load_config(overrides={"train": {"moving_average_decay": value}})) is None
    assert moving_average_decay(Config({})) is None
    assert moving_average_decay(load_config(overrides={"train": {"moving_average_decay": 0.9999}})) == 0.9999
    for bad in (-0.5, 1.0, 1.5, float("nan")):
        with pytest.raises(ValueError):
            moving_average_decay(load_config(overrides={"train": {"moving_average_decay": bad}}))
        with pytest.raises(ValueError):
            check_moving_average_decay(bad)
    assert check_moving_average_decay(None) is None and check_moving_average_decay(0) is None
