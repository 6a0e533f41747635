"""The cross-batch memory without a GPU: the oracle against the definition and against finite differences, its
bounds against an fp32 restatement, the ring model, what the Trainer and the app refuse, the exports, the head's launches on a
stubbed network and the unchanged memory-less step."""
import json
import os

import numpy as np
import pytest
import torch

from facenet_amd import _lib, heads
from facenet_amd.engine import Network
from tests import batch_triplet_oracle as bo
from tests import plan_signature as ps
from tests import xbm_oracle as xo

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


def _rows(n, E, seed):
    x = np.random.default_rng(seed).standard_normal((n, E))
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def _cross64(x, m):
    d = np.asarray(x, np.float64)[:, None, :] - np.asarray(m, np.float64)[None, :, :]
    return (d * d).sum(-1)


def _case(n, M, E, seed, classes=4):
    """Batch and memory rows over a few shared identities, plus one that only the memory has and one that only the batch has."""
    rng = np.random.default_rng(seed)
    x, m = _rows(n, E, seed).astype(np.float32), _rows(M, E, seed + 100).astype(np.float32)
    lab, mlab = rng.integers(0, classes, n), rng.integers(0, classes, M)
    lab[-1], mlab[0] = 900, -7
    return x, m, lab, mlab


# ---- 1. the oracle is the definition -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("soft", [0, 1])
@pytest.mark.parametrize("n,M,valid,seed", [(2, 2, 2, 0), (3, 5, 0, 1), (3, 5, 3, 2), (7, 9, 9, 3), (12, 20, 13, 4)])
def test_oracle_equals_the_literal_loop(n, M, valid, seed, soft):
    x, m, lab, mlab = _case(n, M, 6, seed)
    if n == 2:
        lab, mlab = np.array([0, 1]), np.array([0, 1])
    m[1] = x[0]                                                       # a memory slot that duplicates a batch row: a tie across the sides
    if M > 3:
        m[3] = m[2]                                                   # and two slots that tie
        mlab[3] = mlab[2]
    dist, mdist = bo.sqdist64(x).astype(np.float32), _cross64(x, m).astype(np.float32)
    mdist[:, valid:] = np.nan                                         # stale slots: never looked at
    o = xo.mine(dist, mdist, lab, mlab, valid, 0.2, soft)
    coef, mpick, mcoef, info, loss = xo.literal_loop(dist, mdist, lab, mlab, valid, 0.2, soft)
    assert list(o["info"][:7]) == info and o["info"][7] == 0
    assert np.array_equal(o["mpick"], mpick)
    np.testing.assert_allclose(o["coef"], coef, rtol=0, atol=1e-15)
    np.testing.assert_allclose(o["mcoef"], mcoef, rtol=0, atol=1e-15)
    assert abs(o["loss"] - loss) <= 1e-12 * max(1.0, abs(loss))
    if not soft:
        assert not o["e_coef"].any() and not o["e_mcoef"].any()
    if valid == 0:                                                    # an empty memory is section 31's batch hard
        b = bo.mine(dist, lab, 0.2, 0, soft)
        assert np.array_equal(o["coef"], b["coef"]) and o["loss"] == b["loss"] and list(o["info"][:4]) == list(b["info"][:4])
        assert (o["mpick"] == -1).all() and not o["mcoef"].any()


def test_oracle_smallest_live_case_and_ties():
    """N = M = 2, labels [0, 1] on both sides: no in-batch positive, both rows are anchors through the memory.  The in-batch negative
    (union index 1 - a) ties with nothing; the positive is the memory slot of the row's own label."""
    x, m = _rows(2, 3, 0), _rows(2, 3, 1)
    o = xo.mine(bo.sqdist64(x), _cross64(x, m), [0, 1], [0, 1], 2, 10.0, 0, emb=x, mem=m)
    assert list(o["info"]) == [2, 2, 2, 0, 2, int(o["info"][5]), 2, 0] and list(o["mpick"][:, 0]) == [0, 1]
    assert np.abs(o["demb"]).max() > 0
    # a batch column and a slot at the same distance: the batch wins; two slots: the lower wins
    dist = np.array([[0, 1, 2], [1, 0, 2], [2, 2, 0]], np.float32)
    mdist = np.array([[1, 1, 2, 2], [1, 1, 2, 2], [3, 3, 3, 3]], np.float32)
    o = xo.mine(dist, mdist, [0, 0, 1], [0, 0, 1, 1], 4, 1.5, 0)
    assert o["coef"][0, 1] == 1 and o["coef"][0, 2] == -1 and list(o["mpick"][0]) == [-1, -1]
    o = xo.mine(dist, mdist, [0, 5, 1], [0, 0, 1, 1], 4, 1.5, 0)      # row 0's positives are the tied slots 0 and 1; its nearest negative is batch column 1
    assert list(o["mpick"][0]) == [0, -1] and o["coef"][0, 1] == -1 and o["mcoef"][0, 0] == 1


# ---- 2. the oracle's gradient is the derivative of its loss ----------------------------------------------------------------------
@pytest.mark.parametrize("soft", [0, 1])
@pytest.mark.parametrize("n,M,valid,E,seed", [(8, 11, 11, 5, 21), (9, 14, 6, 4, 22)])
def test_oracle_gradient_matches_central_differences(n, M, valid, E, seed, soft):
    x32, m32, lab, mlab = _case(n, M, E, seed, classes=3)
    x, m = x32.astype(np.float64), m32.astype(np.float64)
    alpha, h = 0.2, 1e-6

    def run(xx, **kw):
        return xo.mine(bo.sqdist64(xx), _cross64(xx, m), lab, mlab, valid, alpha, soft, **kw)
    o = run(x, emb=x, mem=m)
    assert o["Z"] > 0 and o["info"][4] > 0 and o["info"][5] > 0 and np.abs(o["demb"]).max() > 1e-3
    # no argmax / argmin decided by less than 1e-3 and no hinge within 1e-3 of zero: the loss is smooth on the stencil
    du = np.concatenate([bo.sqdist64(x), _cross64(x, m)[:, :valid]], axis=1)
    ulab = np.concatenate([lab, mlab[:valid]])
    for a in range(n):
        same = ulab == lab[a]
        neg = ~same
        same[a] = False
        if not same.any() or not neg.any():
            continue
        dp, dn = np.sort(du[a, same])[::-1], np.sort(du[a, neg])
        assert (len(dp) < 2 or dp[0] - dp[1] >= 1e-3) and (len(dn) < 2 or dn[1] - dn[0] >= 1e-3)
        assert soft or abs(dp[0] - dn[0] + alpha) >= 1e-3
    fd = np.zeros_like(x)
    for r in range(n):
        for e in range(E):
            xp, xm = x.copy(), x.copy()
            xp[r, e] += h
            xm[r, e] -= h
            fd[r, e] = (run(xp)["loss"] - run(xm)["loss"]) / (2 * h)
    np.testing.assert_allclose(o["demb"], fd, rtol=0, atol=2e-8)


def test_oracle_bounds_hold_an_fp32_restatement_and_reject_a_planted_error():
    """The chain restated in fp32 (difference, product, add, each rounded; batch columns ascending, then the memory positive, then the
    memory negative) stays inside e_demb; a planted relative error of 1e-3 does not."""
    n, M, E = 12, 17, 7
    x, m, lab, mlab = _case(n, M, E, 5)
    dist, mdist = bo.sqdist64(x).astype(np.float32), _cross64(x, m).astype(np.float32)
    for soft in (0, 1):
        o = xo.mine(dist, mdist, lab, mlab, 15, 0.2, soft, emb=x, mem=m)
        assert o["info"][4] > 0 and o["info"][5] > 0
        c32, mc32 = o["coef"].astype(np.float32), o["mcoef"].astype(np.float32)
        w = c32 + c32.T
        got = np.zeros((n, E), np.float32)
        for r in range(n):
            acc = np.zeros(E, np.float32)
            for j in range(n):
                if w[r, j] != 0 and j != r:
                    acc = acc + w[r, j] * (x[r] - x[j])
            for k in range(2):
                if o["mpick"][r, k] >= 0 and mc32[r, k] != 0:
                    acc = acc + mc32[r, k] * (x[r] - m[o["mpick"][r, k]])
            got[r] = (acc.astype(np.float64) * 2.0 / o["Z"]).astype(np.float32)
        assert np.all(np.abs(got - o["demb"]) <= o["e_demb"])
        bad = got.copy()
        r, e = np.unravel_index(np.abs(o["demb"]).argmax(), bad.shape)
        bad[r, e] *= 1.001
        assert not np.all(np.abs(bad - o["demb"]) <= o["e_demb"])
        loss32 = np.float32(o["loss"])
        assert abs(float(loss32) - o["loss"]) <= o["e_loss"] < abs(o["loss"]) * 1e-3


# ---- 3. the ring ---------------------------------------------------------------------------------------------------------------
def test_ring_model():
    ring = xo.Ring(7, 2)
    want_emb, want_lab = np.zeros((7, 2), np.float32), np.zeros(7, np.int32)
    states = []
    for call in range(5):
        emb = np.full((3, 2), call + 1, np.float32) + np.arange(3, dtype=np.float32)[:, None] / 8
        ring.enqueue(emb, [10 * call + i for i in range(3)], start=2)
        states.append(ring.state.tolist())
    # calls 0 and 1 are only counted; then cursor 3, 6, and the third stored batch wraps in its middle: slots 6, 0, 1
    assert states == [[0, 0, 1, 0], [0, 0, 2, 0], [3, 3, 3, 0], [6, 6, 4, 0], [2, 7, 5, 0]]
    assert ring.labels.tolist() == [41, 42, 22, 30, 31, 32, 40] and ring.emb[6, 0] == 5.0 and ring.emb[0, 0] == 5.125
    full = xo.Ring(3, 1)
    full.enqueue([[1], [2], [3]], [1, 2, 3])
    full.enqueue([[4], [5], [6]], [4, 5, 6])                          # N = M overwrites everything and the cursor comes back to 0
    assert full.labels.tolist() == [4, 5, 6] and full.state.tolist() == [0, 3, 2, 0]
    with pytest.raises(ValueError):
        full.enqueue(np.zeros((4, 1)), [0] * 4)                       # N > M
    full.state[2] = 2 ** 31 - 1
    full.enqueue([[7]], [7])
    assert full.state.tolist() == [1, 3, 2 ** 31 - 1, 0]              # the call counter saturates


# ---- 4. what the Trainer and the app refuse ----------------------------------------------------------------------------------------
def _check(batch=6, loss="triplet", classes=None, **kw):
    heads.check_loss_arguments(Network(128, allocate=False, device="cpu", nrof_classes=classes), batch, loss, 0.0, 0.95, 0.0, 1.0, **kw)


def test_check_loss_arguments_refusals():
    _check(triplet_strategy="batch_hard", memory_size=6)
    _check(triplet_strategy="batch_hard", memory_size=65536, memory_start=100, soft_margin=True)
    _check(triplet_strategy="batch_all", memory_size=0)
    _check(memory_size=0, memory_start=0)
    for kw in (dict(triplet_strategy="batch_all", memory_size=30), dict(memory_size=30), dict(loss="softmax", classes=10, memory_size=30)):
        with pytest.raises(ValueError, match="cross-batch memory needs"):
            _check(**kw)
    for size in (5, 65537):
        with pytest.raises(ValueError, match=r"memory_size must be in \[batch, 65536\]"):
            _check(triplet_strategy="batch_hard", memory_size=size)
    with pytest.raises(ValueError, match="memory_start must be a non-negative integer"):
        _check(triplet_strategy="batch_hard", memory_size=30, memory_start=-1)
    with pytest.raises(ValueError, match="memory_size must be a non-negative integer"):
        _check(triplet_strategy="batch_hard", memory_size=-30)
    with pytest.raises(ValueError, match="memory_size must be a non-negative integer"):
        _check(triplet_strategy="batch_hard", memory_size=30.5)


class _StubTrainer:
    made = []

    def __init__(self, net, batch, **kw):
        self.net, self.batch, self.kw, self.fed, self.steps, self.captured = net, batch, kw, [], 0, False
        self.rank, self.shadow = 0, None
        self.plan = type("Plan", (), {"images": torch.zeros(batch, 4, 4, 3, dtype=torch.uint8)})()
        _StubTrainer.made.append(self)

    def set_images(self, images, labels=None):
        self.fed.append(None if labels is None else np.asarray(labels).tolist())

    def capture(self):
        self.captured = True

    def step(self):
        self.steps += 1

    def set_learning_rate(self, lr):
        pass

    def loss_value(self):
        return 0.25

    def triplet_stats(self):
        return {"anchors": 4, "terms": 4, "active": 3, "active_fraction": 0.75, "memory_valid": 12, "memory_positives": 2, "memory_negatives": 1}


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


def test_app_memory_settings(app):
    assert app.memory_settings(_cfg()) == (0, 0)
    assert app.memory_settings(_cfg(triplet_strategy="batch_hard", memory_size=4096)) == (4096, 0)
    assert app.memory_settings(_cfg(memory_size=30, memory_start=7)) == (30, 7)
    for bad in (dict(memory_size=-1), dict(memory_size=2.5), dict(memory_size="big"), dict(memory_size=8, memory_start=-2)):
        with pytest.raises(ValueError, match=r"loss\.memory_(size|start) must be a non-negative integer"):
            app.memory_settings(_cfg(**bad))
    for strategy in ({}, dict(triplet_strategy="batch_all"), dict(triplet_strategy="mined")):
        with pytest.raises(ValueError, match="loss.memory_size needs loss.triplet_strategy batch_hard"):
            app.train_tripletloss(_cfg(memory_size=30, **strategy), people_per_batch=2, images_per_person=2)


def test_app_passes_the_memory_on_logs_its_share_and_refuses_unlabelled_pools(app):
    images = torch.zeros(6, 4, 4, 3, dtype=torch.uint8)
    own = [np.array([70, 70, 11, 11, 523, 523]), np.array([8, 8, 70, 70, 9, 9])]
    logs = []
    net, tr = app.train_tripletloss(_cfg(triplet_strategy="batch_hard", memory_size=30, memory_start=1), people_per_batch=3, images_per_person=2,
                                    pools=iter([(images, own[0]), (images, own[1])]), log=logs.append)
    assert tr.kw["memory_size"] == 30 and tr.kw["memory_start"] == 1 and tr.kw["triplet_strategy"] == "batch_hard"
    assert tr.captured and tr.steps == 2 and tr.fed[1:] == [own[0].tolist(), own[1].tolist()]
    assert logs[0] == "triplet strategy: batch_hard, cross-batch memory: 30 rows from step 1"
    assert "active 0.750 (3/4)" in logs[1] and "memory negatives 0.250 (12 rows)" in logs[1] and logs[1].endswith("img/s")
    with pytest.raises(ValueError, match="pools must yield \\(images, labels\\)"):
        app.train_tripletloss(_cfg(triplet_strategy="batch_hard", memory_size=30), people_per_batch=3, images_per_person=2,
                              pools=iter([images]), use_graph=False, log=logs.append)
    # without a memory the app is what it was: no memory arguments reach the Trainer, the line has no memory share
    logs = []
    net, tr = app.train_tripletloss(_cfg(triplet_strategy="batch_hard"), people_per_batch=3, images_per_person=2, pools=iter([images] * 3),
                                    log=logs.append)
    assert "memory_size" not in tr.kw and logs[0] == "triplet strategy: batch_hard" and "memory" not in logs[1]


# ---- 5. the exports ----------------------------------------------------------------------------------------------------------------
def test_exports_and_abi_version():
    lib = _lib.load()
    for name in ("fn_xbm_triplet_fwd_bwd", "fn_xbm_enqueue"):
        assert name in _lib.EXPORTS and hasattr(lib, name)
    assert len(_lib._SIGNATURES["fn_xbm_triplet_fwd_bwd"]) == 19 and len(_lib._SIGNATURES["fn_xbm_enqueue"]) == 10
    assert lib.fn_abi_version() == 1
    header = open(os.path.join(os.path.dirname(GOLDEN), os.pardir, "include", "facenet_hip.h")).read()
    assert "int fn_xbm_triplet_fwd_bwd(" in header and "int fn_xbm_enqueue(" in header


# ---- 6. the head's launches; the memory-less step is unchanged -----------------------------------------------------------------------
HEAD_OPS = ["l2norm_fwd", "pairwise_sqdist", "pairwise_sqdist", "xbm_triplet", "l2norm_bwd", "xbm_enqueue"]


def _trainer_signature(**kw):
    with ps._environ(dict.fromkeys(ps.OPTION_VARS)):
        return ps.trainer_signature(Network(128, allocate=False, device="cpu"), 6, **kw)


def test_memory_head_launches_and_state():
    net = ps._stub_network(Network(128, allocate=False, device="cpu"))
    emb, demb, loss = torch.zeros(6, 128), torch.zeros(6, 128), torch.zeros(4)
    head = heads.xbm_triplet_head(net, emb, demb, loss, 0.2, True, 30, 2)
    assert [op.name for op in head.loss_ops] == HEAD_OPS and not head.pre_ops and not head.final_ops
    assert head.state == ("mem_emb", "mem_labels", "mem_state")
    t = head.tensors
    assert tuple(t["mem_emb"].shape) == (30, 128) and tuple(t["mem_labels"].shape) == (30,) and tuple(t["mem_state"].shape) == (4,)
    assert tuple(t["mem_dist"].shape) == (6, 30) and tuple(t["mpick"].shape) == tuple(t["mcoef"].shape) == (6, 2)
    assert t["mem_labels"].dtype == t["mem_state"].dtype == t["mpick"].dtype == torch.int32 and not t["mem_state"].any()
    sig = _trainer_signature(triplet_strategy="batch_hard", memory_size=30, memory_start=2, soft_margin=True)
    rows = sig["launches"]
    names = [r[0] for r in rows]
    i = names.index("l2norm_fwd")
    assert names[i:i + 6] == HEAD_OPS and "batch_triplet" not in names
    assert [a[1] for a in rows[i + 2][2][:3]] == ["tr.embn", "tr.mem_emb", "tr.mem_dist"] and rows[i + 2][2][4:8] == [6, 30, 128, 2]
    mine = rows[i + 3]
    assert mine[1] == "fn_xbm_triplet_fwd_bwd" and mine[2][13:] == [6, 30, 128, 0.2, 1]
    assert [a[1] for a in mine[2][:13]] == ["tr.embn", "tr.dist", "tr.labels", "tr.mem_emb", "tr.mem_dist", "tr.mem_labels", "tr.mem_state",
                                            "tr.dembn", "tr.loss", "tr.coef", "tr.mpick", "tr.mcoef", "tr.mine_info"]
    enq = rows[i + 5]
    assert enq[1] == "fn_xbm_enqueue" and enq[2][5:] == [6, 30, 128, 2]
    assert [a[1] for a in enq[2][:5]] == ["tr.embn", "tr.labels", "tr.mem_emb", "tr.mem_labels", "tr.mem_state"]
    # the regions order the launches: the mining reads the ring that the enqueue writes, the enqueue reads the state it advances
    ring = {"tr.mem_emb", "tr.mem_labels", "tr.mem_state"}
    assert ring <= {r[0] for r in mine[3]} and not ring & {r[0] for r in mine[4]}
    assert ring == {r[0] for r in enq[4]} and "tr.mem_state" in {r[0] for r in enq[3]}


def test_memory_size_zero_is_todays_trainer():
    with open(os.path.join(GOLDEN, "plan_signatures.json")) as fh:
        golden = json.load(fh)
    assert ps.digest("trainer_triplet", _trainer_signature(loss="triplet", memory_size=0, memory_start=0)) == golden["trainer_triplet"]
    with open(os.path.join(GOLDEN, "batch_triplet_signatures.json")) as fh:
        golden = json.load(fh)
    sig = _trainer_signature(triplet_strategy="batch_hard", memory_size=0)
    assert ps.digest("trainer_batch_hard", sig) == golden["trainer_batch_hard"]
    assert "xbm_enqueue" not in [r[0] for r in sig["launches"]]
