"""Batch-mined triplet losses without a GPU: the oracle against the definition and against finite
differences, what the Trainer refuses, the head's launches pinned to a golden, and the app's config handling on a stubbed trainer."""
import json
import os

import numpy as np
import pytest
import torch

from facenet_amd import heads
from facenet_amd.engine import Network
from tests import batch_triplet_oracle as bo
from tests import plan_signature as ps

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
SETTINGS = [(s, m) for s in (0, 1) for m in (0, 1)]


def _rows(n, E, seed, scale=0.7):
    x = np.random.default_rng(seed).standard_normal((n, E)) * scale
    return x / np.linalg.norm(x, axis=1, keepdims=True)


# ---- 1. the oracle is the definition -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strategy,soft", SETTINGS)
@pytest.mark.parametrize("n,seed", [(2, 0), (3, 1), (7, 2), (12, 3)])
def test_oracle_equals_the_triple_loop(n, seed, strategy, soft):
    labels = [0, 0, 1][:n] if n <= 3 else bo.ragged_labels(n, seed)
    x = _rows(n, 6, seed).astype(np.float32)
    x[n - 1] = x[0]                                                     # a duplicated row: bitwise ties in argmax and argmin
    dist = bo.sqdist64(x).astype(np.float32)
    o = bo.mine(dist, labels, 0.2, strategy, soft)
    coef, counts, loss = bo.triple_loop(dist, labels, 0.2, strategy, soft)
    assert list(o["info"][:3]) == counts and not o["info"][3:].any()
    np.testing.assert_allclose(o["coef"], coef, rtol=0, atol=1e-12)
    assert abs(o["loss"] - loss) <= 1e-12 * max(1.0, abs(loss))
    if not soft:
        assert np.array_equal(o["coef"], coef) and not o["e_coef"].any()


def test_oracle_degenerate_batches_have_no_term():
    for labels in ([0, 0], [0, 1], [5, 5, 5, 5], [1, 2, 3]):
        n = len(labels)
        o = bo.mine(bo.sqdist64(_rows(n, 4, 0)).astype(np.float32), labels, 0.2, 1, 0, emb=_rows(n, 4, 0))
        assert not o["info"].any() and o["loss"] == 0.0 and not o["coef"].any() and not o["demb"].any()


def test_oracle_exact_zero_hinges_are_inactive():
    """Distances on a lattice and alpha = 1: d_ap - d_an + alpha == 0 exactly for the planted triplets, which then count as terms but
    not as active, and leave no coefficient."""
    dist = np.array([[0, 2, 3, 4], [2, 0, 3, 2.5], [3, 3, 0, 1], [4, 2.5, 1, 0]], np.float32)
    o = bo.mine(dist, [0, 0, 1, 1], 1.0, 1, 0)
    # anchor 0: (p=1: 2 - 3 + 1 = 0 inactive), (2 - 4 + 1 < 0); anchor 1: (2 - 3 + 1 = 0), (2 - 2.5 + 1 > 0); anchors 2 and 3: 1 - d_an + 1 < 0
    assert list(o["info"][:4]) == [4, 8, 1, 0]
    assert not o["coef"][0].any() and list(o["coef"][1]) == [1, 0, 0, -1] and not o["coef"][2:].any()
    assert o["Z"] == 1 and o["loss"] == 0.5


# ---- 2. the oracle's gradient is the derivative of its loss ----------------------------------------------------------------------
FD_CASES = [(9, 5, 11), (10, 4, 12)]          # (N, E, seed): committed; the conditions below are asserted, not assumed


@pytest.mark.parametrize("strategy,soft", SETTINGS)
@pytest.mark.parametrize("n,E,seed", FD_CASES)
def test_oracle_gradient_matches_central_differences(n, E, seed, strategy, soft):
    labels = bo.ragged_labels(n, seed, sizes=(2, 3, 1))
    x = _rows(n, E, seed)
    alpha, h = 0.2, 1e-6
    dist = bo.sqdist64(x)
    # no hinge within 1e-3 of zero, no argmax / argmin decided by less than 1e-3: the loss is smooth on the stencil
    for a in range(n):
        same = labels == labels[a]
        neg = ~same
        same[a] = False
        if not same.any() or not neg.any():
            continue
        if strategy == 0:
            dp, dn = np.sort(dist[a, same])[::-1], np.sort(dist[a, neg])
            assert len(dp) < 2 or dp[0] - dp[1] >= 1e-3
            assert len(dn) < 2 or dn[1] - dn[0] >= 1e-3
            hinges = np.array([dp[0] - dn[0] + alpha])
        else:
            hinges = (dist[a, same][:, None] - dist[a, neg][None, :] + alpha).ravel()
        assert soft or np.abs(hinges).min() >= 1e-3
    o = bo.mine(dist, labels, alpha, strategy, soft, emb=x)
    assert o["Z"] > 0 and np.abs(o["demb"]).max() > 1e-3
    fd = np.zeros_like(x)
    for r in range(n):
        for e in range(E):
            xp, xm = x.copy(), x.copy()
            xp[r, e] += h
            xm[r, e] -= h
            fd[r, e] = (bo.mine(bo.sqdist64(xp), labels, alpha, strategy, soft)["loss"] - bo.mine(bo.sqdist64(xm), labels, alpha, strategy, soft)["loss"]) / (2 * h)
    np.testing.assert_allclose(o["demb"], fd, rtol=0, atol=2e-8)


def test_oracle_bounds_hold_an_fp32_restatement_and_reject_a_planted_error():
    """The gather chain restated in fp32 (difference, product, add, each rounded) stays inside e_demb; a planted relative error of
    1e-3 in one element does not."""
    n, E = 12, 7
    labels = bo.ragged_labels(n, 5)
    x = _rows(n, E, 5).astype(np.float32)
    dist = bo.sqdist64(x).astype(np.float32)
    for strategy, soft in SETTINGS:
        o = bo.mine(dist, labels, 0.2, strategy, soft, emb=x)
        c32 = o["coef"].astype(np.float32)
        w = c32 + c32.T
        got = np.zeros((n, E), np.float32)
        for r in range(n):
            acc = np.zeros(E, np.float32)
            for j in range(n):
                if w[r, j] != 0 and j != r:
                    acc = acc + w[r, j] * (x[r] - x[j])
            got[r] = (acc.astype(np.float64) * 2.0 / o["Z"]).astype(np.float32)
        assert np.all(np.abs(got - o["demb"]) <= o["e_demb"])
        bad = got.copy()
        r, e = np.unravel_index(np.abs(o["demb"]).argmax(), bad.shape)
        bad[r, e] *= 1.001
        assert not np.all(np.abs(bad - o["demb"]) <= o["e_demb"])


# ---- 3. what the Trainer refuses -----------------------------------------------------------------------------------------------
def _check(batch=6, loss="triplet", classes=None, **kw):
    net = Network(128, allocate=False, device="cpu", nrof_classes=classes)
    heads.check_loss_arguments(net, batch, loss, 0.0, 0.95, 0.0, 1.0, **kw)


def test_check_loss_arguments_refusals():
    _check()
    _check(triplet_strategy="mined")
    _check(batch=7, triplet_strategy="batch_hard")                       # the multiple-of-3 rule is the mined layout's
    _check(batch=4, triplet_strategy="batch_all", soft_margin=True)
    _check(loss="softmax", classes=10)
    with pytest.raises(ValueError, match="unknown triplet_strategy 'semi_hard'"):
        _check(triplet_strategy="semi_hard")
    with pytest.raises(ValueError, match="belong to triplet training"):
        _check(loss="softmax", classes=10, triplet_strategy="batch_hard")
    with pytest.raises(ValueError, match="belong to triplet training"):
        _check(loss="softmax", classes=10, soft_margin=True)
    with pytest.raises(ValueError, match="soft_margin needs triplet_strategy"):
        _check(soft_margin=True)
    with pytest.raises(ValueError, match="batch must be >= 2"):
        _check(batch=1, triplet_strategy="batch_hard")
    with pytest.raises(ValueError, match="at most 1024 rows"):
        _check(batch=1025, triplet_strategy="batch_all")
    # the old refusals keep their words
    with pytest.raises(ValueError, match=r"unknown loss 'hinge'"):
        _check(loss="hinge")
    with pytest.raises(ValueError, match=r"triplet batches are laid out \(a,p,n,...\): batch must be a multiple of 3"):
        _check(batch=7)
    with pytest.raises(ValueError, match=r"softmax training needs Network\(nrof_classes=...\)"):
        _check(loss="softmax")
    with pytest.raises(ValueError, match="center loss and prelogits-norm loss need class labels: they belong to softmax training"):
        heads.check_loss_arguments(Network(128, allocate=False, device="cpu"), 6, "triplet", 0.1, 0.95, 0.0, 1.0, triplet_strategy="batch_hard")
    with pytest.raises(ValueError, match="the margin softmax needs class labels: it belongs to softmax training"):
        _check(margin_scale=30.0, triplet_strategy="batch_all")


# ---- 4. the head's launches ----------------------------------------------------------------------------------------------------
HEAD_OPS = ["l2norm_fwd", "pairwise_sqdist", "batch_triplet", "l2norm_bwd"]
SIGNATURE_CASES = {"trainer_batch_hard": dict(triplet_strategy="batch_hard"),
                   "trainer_batch_all_soft": dict(triplet_strategy="batch_all", soft_margin=True)}


def _trainer_signature(**kw):
    with ps._environ(dict.fromkeys(ps.OPTION_VARS)):
        return ps.trainer_signature(Network(128, allocate=False, device="cpu"), 6, **kw)


@pytest.mark.parametrize("key", sorted(SIGNATURE_CASES))
def test_batch_triplet_trainer_signature_is_pinned(key):
    """(Record with: python -m tests.test_batch_triplet_host tests/golden/batch_triplet_signatures.json)"""
    with open(os.path.join(GOLDEN, "batch_triplet_signatures.json")) as fh:
        golden = json.load(fh)
    sig = _trainer_signature(**SIGNATURE_CASES[key])
    names = [row[0] for row in sig["launches"]]
    i = names.index("l2norm_fwd")
    assert names[i:i + 4] == HEAD_OPS and "triplet_loss" not in names and "select_triplets" not in names
    row = sig["launches"][i + 2]
    assert row[1] == "fn_batch_triplet_fwd_bwd"
    strategy, soft = row[2][-2:]
    assert (strategy, soft) == ((0, 0) if key == "trainer_batch_hard" else (1, 1))
    assert [a[1] for a in row[2][:7]] == ["tr.embn", "tr.dist", "tr.labels", "tr.dembn", "tr.loss", "tr.coef", "tr.mine_info"]
    assert ps.digest(key, sig) == golden[key]


def test_mined_strategy_is_todays_trainer():
    """triplet_strategy="mined" lowers to the launches pinned before this head existed: the trainer_triplet entry of
    plan_signatures.json (the step) -- and the v1_train_6 entry (the network plan underneath it) still matches as well."""
    with open(os.path.join(GOLDEN, "plan_signatures.json")) as fh:
        golden = json.load(fh)
    sig = _trainer_signature(loss="triplet", triplet_strategy="mined")
    assert ps.digest("trainer_triplet", sig) == golden["trainer_triplet"]
    assert ps.digest("trainer_triplet", _trainer_signature(loss="triplet")) == golden["trainer_triplet"]
    assert ps.digest("v1_train_6") == golden["v1_train_6"]
    names = [row[0] for row in sig["launches"]]
    assert "triplet_loss" in names and "batch_triplet" not in names and "pairwise_sqdist" not in names


def test_head_carries_no_state():
    net = ps._stub_network(Network(128, allocate=False, device="cpu"))
    emb, demb, loss = torch.zeros(6, 128), torch.zeros(6, 128), torch.zeros(4)
    head = heads.batch_triplet_head(net, emb, demb, loss, 0.2, "batch_all", False)
    assert head.state == () and not head.pre_ops and not head.final_ops
    assert [op.name for op in head.loss_ops] == HEAD_OPS
    assert sorted(head.tensors) == ["coef", "dembn", "dist", "embn", "labels", "mine_info"]
    assert head.tensors["labels"].dtype == torch.int32 and tuple(head.tensors["labels"].shape) == (6,)
    assert tuple(head.tensors["dist"].shape) == tuple(head.tensors["coef"].shape) == (6, 6)


# ---- 5. the app's config handling --------------------------------------------------------------------------------------------------
class _StubTrainer:
    made = []

    def __init__(self, net, batch, **kw):
        self.net, self.batch, self.kw, self.fed, self.steps, self.captured = net, batch, kw, [], 0, False
        self.rank, self.shadow = 0, None
        self.plan = type("Plan", (), {"images": torch.zeros(batch, 4, 4, 3, dtype=torch.uint8)})()
        _StubTrainer.made.append(self)

    def set_images(self, images, labels=None):
        self.fed.append((tuple(images.shape), None if labels is None else np.asarray(labels).tolist()))

    def capture(self):
        self.captured = True

    def step(self):
        self.steps += 1

    def set_learning_rate(self, lr):
        pass

    def loss_value(self):
        return 0.25

    def triplet_stats(self):
        return {"anchors": 4, "terms": 8, "active": 6, "active_fraction": 0.75}


@pytest.fixture
def app(monkeypatch):
    from facenet_amd.apps import train_tripletloss as mod
    _StubTrainer.made = []
    monkeypatch.setattr(mod, "Trainer", _StubTrainer)
    monkeypatch.setattr(mod, "build_network", lambda *a, **k: "net")
    monkeypatch.setattr(mod.torch.cuda, "synchronize", lambda *a, **k: None)
    return mod


def _cfg(**loss):
    from facenet_amd.config import load_config
    return load_config(overrides={"image": {"size": 4}, "loss": loss, "train": {"epoch": {"nrof_epochs": 1, "size": 2}, "learning_rate": {"value": 0.01}}})


def test_app_settings_parsing(app):
    assert app.triplet_settings(_cfg()) == ("mined", False)
    assert app.triplet_settings(_cfg(triplet_strategy="mined")) == ("mined", False)
    assert app.triplet_settings(_cfg(triplet_strategy="batch_hard")) == ("batch_hard", False)
    assert app.triplet_settings(_cfg(triplet_strategy="batch_all", soft_margin=True)) == ("batch_all", True)
    with pytest.raises(ValueError, match="loss.triplet_strategy"):
        app.triplet_settings(_cfg(triplet_strategy="hardest"))
    with pytest.raises(ValueError, match="loss.soft_margin needs"):
        app.train_tripletloss(_cfg(soft_margin=True), people_per_batch=2, images_per_person=2)


@pytest.mark.parametrize("use_graph", [False, True])
def test_app_batch_strategy_default_labels_and_labelled_pools(app, use_graph):
    logs = []
    P, K = 3, 2
    images = torch.zeros(P * K, 4, 4, 3, dtype=torch.uint8)
    own = np.array([7, 7, -1, 9, 9, -1])
    pools = iter([images, (images, own), images])
    net, tr = app.train_tripletloss(_cfg(triplet_strategy="batch_all", soft_margin=True, alpha=0.3), people_per_batch=P, images_per_person=K,
                                    nrof_triplets=30, pools=pools, use_graph=use_graph, log=logs.append)
    assert _StubTrainer.made == [tr] and tr.batch == P * K             # the whole batch, not 3 * nrof_triplets; no TripletMiner
    assert tr.kw["triplet_strategy"] == "batch_all" and tr.kw["soft_margin"] is True and tr.kw["loss"] == "triplet" and tr.kw["alpha"] == 0.3
    fed = tr.fed[1:] if use_graph else tr.fed                          # (the batch capture()'s warm-up step runs on)
    assert tr.captured == use_graph and tr.steps == 2 and len(fed) == 2
    assert fed[0] == ((6, 4, 4, 3), [0, 0, 1, 1, 2, 2]) and fed[1] == ((6, 4, 4, 3), own.tolist())
    assert logs[0] == "triplet strategy: batch_all, soft margin"
    assert "active 0.750 (6/8)" in logs[1] and "triplet loss 0.2500" in logs[1] and logs[1].endswith("img/s") and len(logs) == 2


if __name__ == "__main__":      # python -m tests.test_batch_triplet_host OUT.json: record the head's signatures with this checkout
    import sys
    with open(sys.argv[1], "w") as out:
        json.dump({k: ps.digest(k, _trainer_signature(**kw)) for k, kw in SIGNATURE_CASES.items()}, out, indent=1, sort_keys=True)
        out.write("\n")
