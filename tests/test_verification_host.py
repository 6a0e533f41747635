"""The host side of the exact verification curve: the descent of facenet_amd.statistics driven by the
oracle's NumPy histogram in place of fn_pair_key_histogram, against the sort-based answers of tests/verification_oracle.py."""
import numpy as np
import pytest

from facenet_amd import statistics as st
from tests import pair_lattice as pl
from tests import verification_oracle as vo

FARS = [0, 1e-3, 1e-2, 0.1, 0.5, 1]


class Counting:
    """The stand-in for the kernel: the oracle's histogram of two key lists; remembers every pass's windows."""

    def __init__(self, gen, imp):
        self.gen, self.imp, self.calls = np.sort(np.asarray(gen, np.int64)), np.sort(np.asarray(imp, np.int64)), []

    def __call__(self, lo, shift):
        assert 1 <= len(lo) == len(shift) <= 8 and all(0 <= s <= 22 for s in shift) and all(0 <= l < 2 ** 32 for l in lo)
        self.calls.append((list(lo), list(shift)))
        return vo.histogram(self.gen, self.imp, lo, shift)

    def curve(self, metric=0):
        return st.VerificationCurve.from_histogram(self, len(self.gen), len(self.imp), metric)


def check(gen, imp, fars=FARS, metric=0, max_passes=4):
    h = Counting(gen, imp)
    curve = h.curve(metric)
    got = curve.tar_at_far(fars)
    want = [vo.tar_at_far(h.gen, h.imp, f) for f in fars]
    for g, w in zip(got, want):
        assert np.float32(g["threshold"]).tobytes() == np.float32(w["threshold"]).tobytes(), (g, w)
        assert g == w
        assert type(g["false_accepts"]) is int and type(g["true_accepts"]) is int
    assert curve.eer() == vo.eer(h.gen, h.imp)
    assert curve.nrof_passes == len(h.calls) <= max_passes, h.calls
    keys, ta, fa = curve.roc_counts()
    assert keys[0] == 0 and keys == sorted(set(keys)) and (ta[0], fa[0]) == (0, 0) and (ta[-1], fa[-1]) == (len(h.gen), len(h.imp))
    assert (ta, fa) == vo.roc_at(h.gen, h.imp, keys)
    far, tar, thr = curve.roc()
    assert thr.dtype == np.float32 and np.array_equal(thr.view(np.uint32), np.array(keys, np.uint32))
    assert np.array_equal(far, np.array(fa) / len(h.imp)) and np.array_equal(tar, np.array(ta) / len(h.gen))
    auc, auc_lo, auc_hi = curve.auc()
    exact = vo.auc(h.gen, h.imp)
    assert auc_lo <= float(exact) <= auc_hi and auc == pytest.approx((auc_lo + auc_hi) / 2, abs=1e-15) and 0 <= auc_lo <= auc_hi <= 1
    assert len(h.calls) == curve.nrof_passes                # the curve and its area need no further pass
    d = curve.dict()
    assert d["nrof_genuine"] == len(h.gen) and d["nrof_impostor"] == len(h.imp) and d["tar_at_far"] == want and d["auc"] == auc
    text = repr(curve)
    assert text.startswith("VerificationCurve\nmetric: {}\n".format(metric)) and text.count("TAR @ FAR = ") == len(set(fars))
    return curve, h


def _random_keys(seed, n_gen, n_imp):
    rng = np.random.default_rng(seed)
    gen = np.abs(rng.normal(0.6, 0.3, n_gen)).clip(0, 4).astype(np.float32)
    imp = rng.normal(2.0, 0.15, n_imp).clip(0, 4).astype(np.float32)
    return vo.keys_of(gen), vo.keys_of(imp)


def test_first_pass_is_the_octaves_down_from_four():
    lo, shift = st.FIRST_WINDOWS
    assert len(lo) == 8 and lo[0] == vo.f32_key(2.0) and lo[-1] == vo.f32_key(2.0 ** -6) and set(shift) == {13}
    assert all(a - b == 1024 << 13 for a, b in zip(lo, lo[1:])) and lo[0] + (1024 << 13) == vo.f32_key(4.0) == st.KEY_TOP[0]
    assert st.KEY_TOP[1] == vo.f32_key(np.pi) and st.KEY_TOP[1] < st.KEY_TOP[0]
    assert st.f32_key(1.5) == vo.f32_key(1.5) and st.key_f32(vo.f32_key(0.3)) == float(np.float32(0.3))


@pytest.mark.parametrize("metric", [0, 1])
def test_random_keys_take_three_passes(metric):
    gen, imp = _random_keys(1, 3000, 100000)
    if metric == 1:
        gen, imp = np.minimum(gen, st.KEY_TOP[1]), np.minimum(imp, st.KEY_TOP[1])
    curve, h = check(gen, imp, metric=metric, max_passes=3)
    assert h.calls[0] == (st.FIRST_WINDOWS[0], st.FIRST_WINDOWS[1])
    assert all(len(lo) <= 8 for lo, _ in h.calls) and curve.nrof_groups == 1


def test_all_keys_equal():
    k = vo.f32_key(1.0)
    curve, _ = check([k] * 5, [k] * 40)
    assert curve.eer()["eer_threshold"] == vo.key_f32(k + 1) and curve.tar_at_far([0.5])[0]["false_accepts"] == 0
    assert curve.auc() == (0.5, 0.0, 1.0)


def test_only_zero_and_four():
    top = vo.f32_key(4.0)
    curve, _ = check([0] * 30 + [top] * 3, [0] * 7 + [top] * 93)
    rec = curve.tar_at_far([0.07, 0.5])
    assert rec[0]["threshold"] == 4.0 and rec[0]["false_accepts"] == 7 and rec[1]["threshold"] == 4.0
    assert curve.tar_at_far([0.069])[0]["threshold"] == 0.0
    check([top] * 4, [top] * 9)                             # nothing below the top key at all


def test_target_below_the_first_windows():
    """Distances under 2^-6 are one count of the first pass: three further passes of shift 20, 10 and 0."""
    rng = np.random.default_rng(3)
    gen = vo.keys_of(rng.uniform(0, 1e-3, 500).astype(np.float32))
    imp = vo.keys_of(np.concatenate([rng.uniform(1e-4, 1e-2, 4000), rng.uniform(1.5, 2.5, 1000)]).astype(np.float32))
    curve, h = check(gen, imp)
    assert max(imp[:4000]) < st.FIRST_WINDOWS[0][-1] and curve.nrof_passes == 4
    assert [max(s) for _, s in h.calls[1:]] == [20, 10, 0]


def test_single_impostor():
    gen, _ = _random_keys(4, 50, 1)
    k = vo.f32_key(1.75)
    curve, _ = check(gen, [k])
    assert [r["threshold"] for r in curve.tar_at_far([0, 0.999, 1])] == [1.75, 1.75, float("inf")]


def test_lattice_distances_tie_massively():
    _, starts, H = pl.lattice_classes([5, 33, 2, 70], seed=4, flips=32, scale=1 + 2.0 ** -5)
    gen, imp = vo.lattice_keys(H, starts, 64, 1 + 2.0 ** -5)
    assert gen[0] == 0 and gen[-1] == vo.f32_key(4.0) and len(np.unique(imp)) < 80 and len(imp) > 3000
    curve, _ = check(gen, imp)
    rec = curve.tar_at_far([0.3])[0]
    assert rec["false_accepts"] < int(0.3 * len(imp))       # ties: the count stays below m


def test_far_zero_one_and_exact_products():
    gen, imp = _random_keys(5, 400, 8000)
    curve, _ = check(gen, imp, fars=[0, 0.125, 0.25, 1])    # 0.125 * 8000 = 1000 exactly
    r0, r1, _, r3 = curve.tar_at_far([0, 0.125, 0.25, 1])
    assert r0["threshold"] == vo.key_f32(int(np.min(imp))) and r0["false_accepts"] == 0
    assert r1["threshold"] == vo.key_f32(int(np.sort(imp)[1000])) and r1["false_accepts"] == 1000        # no tie there
    assert r3 == {"far_target": 1.0, "threshold": float("inf"), "false_accepts": 8000, "true_accepts": 400, "far": 1.0, "tar": 1.0}
    assert curve.threshold_at_far(0.125) == r1["threshold"]


def test_nine_targets_run_in_two_groups():
    gen, imp = _random_keys(6, 1000, 50000)
    fars = [1e-4, 3e-4, 1e-3, 3e-3, 1e-2, 3e-2, 0.1, 0.3, 0.6]
    h = Counting(gen, imp)
    curve = h.curve()
    got = curve.tar_at_far(fars)
    assert got == [vo.tar_at_far(h.gen, h.imp, f) for f in fars] and curve.eer() == vo.eer(h.gen, h.imp)
    assert curve.nrof_groups == 2 and all(len(lo) <= 8 for lo, _ in h.calls)
    assert len(h.calls[1][0]) == 8 and curve.nrof_passes == len(h.calls) <= 1 + 2 * 2
    before = len(h.calls)
    assert curve.tar_at_far(fars[2:5]) == got[2:5] and curve.eer() and len(h.calls) == before        # known thresholds cost nothing


def test_rejected_inputs():
    gen, imp = _random_keys(7, 10, 10)
    with pytest.raises(ValueError):
        st.VerificationCurve.from_histogram(Counting([], imp), 0, 10)
    with pytest.raises(ValueError):
        st.VerificationCurve.from_histogram(Counting(gen, []), 10, 0)
    with pytest.raises(ValueError):
        st.VerificationCurve.from_histogram(Counting(gen, imp), 10, 10, metric=2)
    # no launch and no device for one class, or for classes of one row
    with pytest.raises(ValueError):
        st.VerificationCurve(np.eye(4, dtype=np.float32), [3, 3, 3, 3], device="cpu")
    with pytest.raises(ValueError):
        st.VerificationCurve(np.eye(4, dtype=np.float32), [0, 1, 2, 3], device="cpu")
    h = Counting(gen, imp)
    curve = h.curve()
    for bad in ([0.1, 0.01], [-1e-9], [0.5, 1.0000001], [float("nan")]):
        with pytest.raises(ValueError):
            curve.tar_at_far(bad)
    assert h.calls == []


def test_the_config_key_is_off_by_default(tmp_path):
    from facenet_amd.apps.validate import DEFAULTS, load_options
    assert DEFAULTS["validate"] == {"nrof_folds": 10, "metric": 0, "far_target": 0.001}
    opt = load_options(overrides={"model": {"path": str(tmp_path)}})
    assert opt.validate.as_dict == DEFAULTS["validate"]
    assert st.verification_curve(None, None, opt.validate) is None                    # nothing is looked at
    opt = load_options(overrides={"model": {"path": str(tmp_path)}, "validate": {"far_targets": None}})
    assert st.verification_curve(None, None, opt.validate) is None
    opt = load_options(overrides={"model": {"path": str(tmp_path)}, "validate": {"far_targets": [0.01, 0.001]}})
    assert opt.validate.far_targets == [0.01, 0.001] and opt.validate.nrof_folds == 10


# ---- the callback's wiring (the curve itself is a stub here; tests/test_gpu_verification.py runs the real one) ----------------------
class _Model:
    def __init__(self, path=None):
        self.path = path

    def __call__(self, images):
        return np.asarray(images, np.float32).reshape(len(images), -1)[:, :2]


class _Report:
    dict = {"stub": 1}

    def __init__(self, embeddings, labels, config):
        self.n = len(labels)

    def __repr__(self):
        return "stub report {}\n".format(self.n)

    def write_report(self, file):
        with open(file, "at") as f:
            f.write(str(self))


def test_callback_appends_the_curve_only_with_the_key(tmp_path, monkeypatch):
    from facenet_amd import callbacks
    from facenet_amd.config import Config
    data = [(np.ones((3, 2, 2, 3), np.uint8), np.array([0, 0, 1]))]
    seen = []

    def stub_curve(embeddings, labels, config, device="cuda"):
        seen.append((len(labels), config.far_targets))
        return None if isinstance(config.far_targets, Config) else "stub curve {}\n".format(config.far_targets)

    monkeypatch.setattr(st, "verification_curve", stub_curve)
    for k, validate in enumerate(({"metric": 0, "nrof_folds": 2, "far_target": 1e-3},
                                  {"metric": 0, "nrof_folds": 2, "far_target": 1e-3, "far_targets": [0.01]})):
        lines, model = [], _Model(tmp_path / f"run{k}")
        cb = callbacks.ValidateCallback(model, data, 1, 1, Config({"validate": validate}), log=lambda s: lines.append(str(s)),
                                        statistic=_Report)
        report = cb.on_epoch_end(0)
        text = (tmp_path / f"run{k}" / "report.txt").read_text()
        if k == 0:
            assert not hasattr(report, "curve") and text == "stub report 3\n" and not any("stub curve" in l for l in lines)
        else:
            assert report.curve == "stub curve [0.01]\n" and text == "stub report 3\n" + 64 * "-" + "\nstub curve [0.01]\n"
            assert lines.index("stub curve [0.01]\n") == lines.index("stub report 3\n") + 1
    assert [n for n, _ in seen] == [3, 3]
