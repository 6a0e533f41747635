"""The update rules of train.optimizer on the host: the fp32 oracle against its float64 form, the Keras
checkpoint names of every rule's slots, and the config helper of the training apps."""
import numpy as np
import pytest

from facenet_amd import keras_names
from facenet_amd.config import Config, load_config
from facenet_amd.train import OPTIMIZERS, check_optimizer, optimizer_name
from tests import optimizer_oracle as oo


@pytest.mark.parametrize("name", oo.RULES)
def test_oracle_matches_the_float64_form_across_a_learning_rate_change(name):
    rng = np.random.default_rng(len(name))
    n, n_decay = 4000, 2500
    w = rng.standard_normal(n).astype(np.float32)
    s32, s64 = oo.initial_slots(name, n), [x.astype(np.float64) for x in oo.initial_slots(name, n)]
    w32, w64 = w.copy(), w.astype(np.float64)
    for k, lr in enumerate((0.05, 0.05, 0.05, 0.005, 0.005, 0.0005)):
        G = (rng.standard_normal(n) * 0.1).astype(np.float32)
        w32, s32 = oo.step(name, w32, G, s32, lr, grad_scale=0.5, l2=5e-4, n_decay=n_decay)
        w64, s64 = oo.step64(name, w64, G, s64, lr, grad_scale=0.5, l2=5e-4, n_decay=n_decay)
        assert w32.dtype == np.float32 and all(x.dtype == np.float32 for x in s32)
        np.testing.assert_allclose(w32, w64, rtol=1e-5, atol=1e-6 * (k + 1))
        for a, b in zip(s32, s64):
            np.testing.assert_allclose(a, b, rtol=1e-4, atol=1e-7 * (k + 1))
    assert not np.array_equal(w32, w)


def test_oracle_first_steps_by_hand():
    g = np.array([0.5, -2.0, 0.0, 1.0], np.float32)
    w = np.array([1.0, 2.0, 3.0, -4.0], np.float32)
    F = np.float32
    # Adagrad starts its accumulator at 0.1 (Keras initial_accumulator_value), eps 1e-7
    w1, (a,) = oo.step("ADAGRAD", w, g, oo.initial_slots("ADAGRAD", 4), 0.1)
    assert np.array_equal(a, F(0.1) + g * g)
    assert np.array_equal(w1, w - (F(0.1) * g) / (np.sqrt(a) + F(1e-7)))
    # Nesterov momentum from zero: acc = -lr g, w += mu acc - lr g = -(1 + mu) lr g
    w1, (acc,) = oo.step("MOM", w, g, oo.initial_slots("MOM", 4), 0.1)
    assert np.array_equal(acc, -(F(0.1) * g))
    assert np.array_equal(w1, w + (F(0.9) * acc - F(0.1) * g))
    # Keras RMSprop: rms starts at 0 (TF1 starts it at 1), eps 1.0
    w1, (ms, mom) = oo.step("RMSPROP", w, g, oo.initial_slots("RMSPROP", 4), 0.1)
    assert np.array_equal(ms, (F(1) - F(0.9)) * (g * g)) and np.array_equal(w1, w - mom)
    # Adadelta with lr 1 and zero accumulators moves by sqrt(eps) / sqrt(ag + eps) * g
    w1, (ag, av) = oo.step("ADADELTA", w, g, oo.initial_slots("ADADELTA", 4), 1.0)
    u = np.sqrt(F(1e-6)) / np.sqrt(ag + F(1e-6)) * g
    assert np.array_equal(w1, w - u) and np.array_equal(av, (F(1) - F(0.9)) * (u * u))
    # the L2 term joins g on the first n_decay elements only
    assert np.array_equal(oo.gradient(g, w, 2.0, 0.25, 2), np.array([1.0 + 0.5, -4.0 + 1.0, 0.0, 2.0], np.float32))


def test_the_rule_table():
    assert list(OPTIMIZERS) == ["ADAGRAD", "ADADELTA", "ADAM", "RMSPROP", "MOM"]
    assert {k: r.keras for k, r in OPTIMIZERS.items()} == {"ADAGRAD": "Adagrad", "ADADELTA": "Adadelta", "ADAM": "Adam",
                                                          "RMSPROP": "RMSprop", "MOM": "SGD"}
    assert {k: r.slots for k, r in OPTIMIZERS.items()} == {
        "ADAGRAD": (("accumulator", 0.1),), "ADADELTA": (("accum_grad", 0.0), ("accum_var", 0.0)), "ADAM": (("m", 0.0), ("v", 0.0)),
        "RMSPROP": (("rms", 0.0), ("momentum", 0.0)), "MOM": (("momentum", 0.0),)}
    assert len({r.code for r in OPTIMIZERS.values()}) == 5 and OPTIMIZERS["ADAM"].code == 0
    assert [OPTIMIZERS[k].op for k in oo.RULES] == ["adagrad_keras", "adadelta_keras", "rmsprop_keras", "sgd_keras"]


@pytest.mark.parametrize("family", ["v1", "v2"])
def test_slot_and_key_names(family):
    if family == "v1":
        from facenet_amd.engine import Network
        net = Network(embedding_size=128, nrof_classes=7, allocate=False)
    else:
        from facenet_amd.engine_v2 import NetworkV2
        net = NetworkV2(128, config={"repeat": [1, 1, 1]}, nrof_classes=7, allocate=False)
    table = net.variable_table()
    model = {k for k, _ in table}
    trainable = [k for k, i in table if not i.endswith(("moving_mean", "moving_variance"))]
    shadows = {keras_names.moving_average_name(k) for k in trainable}
    # Adam's names are the default
    assert keras_names.optimizer_slot_names(trainable[0]) == keras_names.optimizer_slot_names(trainable[0], "Adam", ("m", "v"))
    every = set()
    for name, r in OPTIMIZERS.items():
        slot_names = tuple(s for s, _ in r.slots)
        names = [keras_names.optimizer_slot_names(k, r.keras, slot_names) for k in trainable]
        flat = {x for t in names for x in t}
        assert len(flat) == len(slot_names) * len(trainable)
        assert all(x.startswith(r.keras + "/") and x.endswith(tuple(f"/{s}:0" for s in slot_names)) for x in flat)
        assert not flat & model and not flat & shadows and not flat & every
        every |= flat
    base = trainable[0][:-2] if trainable[0].endswith(":0") else trainable[0]
    assert keras_names.optimizer_slot_names(trainable[0], "Adagrad", ("accumulator",)) == (f"Adagrad/{base}/accumulator:0",)
    assert keras_names.optimizer_slot_names(trainable[0], "RMSprop", ("rms", "momentum")) == (f"RMSprop/{base}/rms:0",
                                                                                          f"RMSprop/{base}/momentum:0")
    assert keras_names.optimizer_slot_names(trainable[0], "SGD", ("momentum",)) == (f"SGD/{base}/momentum:0",)


def test_config_helper():
    assert optimizer_name(load_config()) == "ADAM"                                     # the default
    assert optimizer_name(Config({})) == "ADAM"                                        # a missing key
    assert optimizer_name(load_config(overrides={"train": {"optimizer": None}})) == "ADAM"
    for name in OPTIMIZERS:
        assert optimizer_name(load_config(overrides={"train": {"optimizer": name}})) == name
    for bad in ("RMSProp", "adam", "SGD", "", "LARS", 3):
        with pytest.raises(ValueError, match="Invalid optimization algorithm"):
            optimizer_name(load_config(overrides={"train": {"optimizer": bad}}))
        with pytest.raises(ValueError, match="Invalid optimization algorithm"):
            check_optimizer(bad)


@pytest.mark.parametrize("app", ["softmax", "triplet"])
def test_apps_reject_a_bad_name_before_building_the_network(app, monkeypatch):
    from facenet_amd.apps import train_softmax as ts, train_tripletloss as tt
    mod = ts if app == "softmax" else tt

    def no_network(*a, **k):
        raise AssertionError("the network was built before the optimizer name was checked")
    monkeypatch.setattr(mod, "build_network", no_network)
    cfg = load_config(overrides={"batch_size": 6, "train": {"optimizer": "RMSProp", "epoch": {"nrof_epochs": 1, "size": 1}}})
    with pytest.raises(ValueError, match="Invalid optimization algorithm 'RMSProp'"):
        if app == "softmax":
            ts.train_softmax(cfg, 7, log=lambda *_: None)
        else:
            tt.train_tripletloss(cfg, log=lambda *_: None)
