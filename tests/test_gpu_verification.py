"""fn_pair_key_histogram and VerificationCurve on the device against tests/verification_oracle.py: every
word of the histogram, every threshold bit for bit, every count as an integer.  Every launch of the primitive goes through the C
ABI with guard words behind `out` and `range`."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from facenet_amd import _lib
from facenet_amd import statistics as st
from tests import pair_lattice as pl
from tests import verification_oracle as vo

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 8
FILL = -77
B = st.KEY_BINS
FARS = [0, 1e-3, 1e-2, 0.1, 0.5, 1]
POOLS = [pl.RANDOM_POOLS[0], ([70, 45], 96), ([65, 64, 1], 4), ([3] * 20, 512)]
POOL_IDS = ["7-classes-E128", "70-45-E96", "65-64-1-E4", "20x3-E512"]
SCALE = 1 + 2.0 ** -5


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def launch(emb_ptr, cls_ptr, C, E, metric, lo, shift, R, out_ptr, rng_ptr):
    lib = _lib.load()
    return lib.fn_pair_key_histogram(emb_ptr, cls_ptr, C, E, metric, (ctypes.c_uint32 * max(len(lo), 1))(*lo),
                                     (ctypes.c_int32 * max(len(shift), 1))(*shift), R, out_ptr, rng_ptr,
                                     torch.cuda.current_stream().cuda_stream)


def run_hist(emb, starts, metric, lo, shift):
    """-> (out uint64 [R, 2, B + 2], (min, max) of the dots); asserts that nothing behind `out` and `range` was written."""
    R, words = len(lo), len(lo) * 2 * (B + 2)
    e, s = _dev(emb, np.float32), _dev(starts, np.int32)
    out = torch.full((words + GUARD,), FILL, dtype=torch.int64, device=DEV)
    out[:words] = 0                                                    # the caller zeroes out
    rng = torch.full((2 + GUARD,), FILL, dtype=torch.int32, device=DEV)
    rc = launch(e.data_ptr(), s.data_ptr(), len(starts) - 1, emb.shape[1], metric, lo, shift, R, out.data_ptr(), rng.data_ptr())
    assert rc == 0, _lib.load().fn_last_error()
    torch.cuda.synchronize()
    o, r = out.cpu().numpy(), rng.cpu().tolist()
    assert (o[words:] == FILL).all() and r[2:] == [FILL] * GUARD
    return o[:words].view(np.uint64).reshape(R, 2, B + 2), (st._decode_ord(r[0]), st._decode_ord(r[1]))


def mixed_windows(gen, imp):
    """Eight windows: single keys around a populated impostor key, one above every key, one below every positive key, three that
    overlap, the whole range at the largest shift, the first pass's top octave."""
    k = int(imp[len(imp) // 2])
    lo = [k - 5, vo.f32_key(4.0) + 1, 1, vo.f32_key(1.0), vo.f32_key(1.5), vo.f32_key(0.5), 0, vo.f32_key(2.0)]
    return lo, [0, 0, 0, 13, 12, 14, 22, 13]


def assert_same_words(got, want):
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (len(bad), [(tuple(int(v) for v in i), int(got[tuple(i)]), int(want[tuple(i)])) for i in bad[:6]])


@functools.lru_cache(maxsize=None)
def random_pool(sizes, E):
    """(emb sorted by class, starts, labels, (genuine, impostor) metric-0 keys of the host's fp32 chain)."""
    emb, starts, labels = pl.sorted_pool(list(sizes), E)
    return emb, starts, labels, vo.chain_keys(emb, starts)


@functools.lru_cache(maxsize=None)
def lattice_pool():
    emb, starts, H = pl.lattice_classes([5, 33, 2, 70, 1, 65], seed=21, flips=32, E_pad=4, scale=SCALE)
    gen, imp = vo.lattice_keys(H, starts, 64, SCALE)
    assert gen[0] == 0 and gen[-1] == vo.f32_key(4.0) and pl.want_range(pl.exact_dots(H, 64, SCALE), starts) == (-SCALE ** 2, SCALE ** 2)
    return emb, starts, (gen, imp), pl.exact_dots(H, 64, SCALE)


def gallery_keys(emb, starts, labels, metric):
    """The keys of the distances an existing consumer of pair_tiles.h reports: the radius self-join at eps = +inf returns every
    other row of every row with its distance (fn_radius_fill).  fn_pairwise_sqdist is NOT such a source: it shares pair_distance
    only and sums its dot products by wavefront reduction, so its distances differ from the chain's in the last bits (on the first
    pool the smallest impostor distance reads 0x3fb75782 there and 0x3fb75780 in the chain)."""
    from facenet_amd.recognize import Gallery
    n = len(emb)
    offsets, rows, dist = Gallery(emb, labels, metric=metric, device=DEV).neighbours(np.float32(np.inf))
    offsets, rows, dist = offsets.cpu().numpy(), rows.cpu().numpy(), dist.cpu().numpy()
    assert offsets[-1] == n * (n - 1) and np.all(np.diff(offsets) == n - 1)
    keys = np.zeros((n, n), np.int64)
    keys[np.repeat(np.arange(n), n - 1), rows] = vo.keys_of(dist)
    assert np.array_equal(keys, keys.T)
    return vo.split(keys, starts)


@functools.lru_cache(maxsize=None)
def device_keys(sizes, E, metric):
    emb, starts, labels, _ = random_pool(sizes, E)
    return gallery_keys(emb, starts, labels, metric)


# ---- the primitive: every word of out ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sizes,E", POOLS, ids=POOL_IDS)
def test_histogram_words_random_rows(sizes, E):
    emb, starts, _, (gen, imp) = random_pool(tuple(sizes), E)
    for lo, shift in (([0], [21]), mixed_windows(gen, imp)):
        got, rng = run_hist(emb, starts, 0, lo, shift)
        want = vo.histogram(gen, imp, lo, shift)
        assert_same_words(got, want)
        assert int(got[0, 1, :B].sum()) + int(got[0, 1, B]) <= len(imp) == int(got[0, 1, B + 1])
    assert got[0, 1, 5] >= 1 and got[1].sum() == got[1, :, B:].sum()     # the populated key has its own bin; nothing above 4.0
    dots = pl.fp32_chain(emb, emb)
    a, b, _ = pl._pairs(starts)
    assert rng == (float(dots[a, b].min()), float(dots[a, b].max()))


def test_histogram_words_lattice_rows():
    """Duplicates (d = 0), negated rows (d = 4.0) and |s| > 1 (the clamp) under massive ties; E = 68 has a partial chunk."""
    emb, starts, (gen, imp), dots = lattice_pool()
    for lo, shift in (([0], [21]), mixed_windows(gen, imp), st.FIRST_WINDOWS):
        got, rng = run_hist(emb, starts, 0, lo, shift)
        assert_same_words(got, vo.histogram(gen, imp, lo, shift))
        assert rng == pl.want_range(dots, starts)
    top = got[0, 0]                                                      # the octave [2, 4): d = 4.0 is beyond its last bin
    assert int(top[B + 1]) - int(top[B]) - int(top[:B].sum()) == np.count_nonzero(gen == vo.f32_key(4.0)) > 0


def test_histogram_words_many_class_pairs_per_workgroup():
    """300 classes: every workgroup of the class-pair walk takes several class pairs (44 850 off-diagonal ones over 2048
    workgroups, 300 diagonal ones over 256), so its counters and its below / total registers carry over from pair to pair."""
    _, emb, starts, H = pl.many_class_pool()
    gen, imp = vo.lattice_keys(H, starts, 16)
    assert (len(starts) - 1, len(gen), len(imp)) == (300, 1050, 338850)
    for lo, shift in (([0], [21]), mixed_windows(gen, imp), st.FIRST_WINDOWS):
        got, rng = run_hist(emb, starts, 0, lo, shift)
        assert_same_words(got, vo.histogram(gen, imp, lo, shift))
        assert rng == pl.want_range(pl.exact_dots(H, 16), starts)
        assert (int(got[0, 0, B + 1]), int(got[0, 1, B + 1])) == (1050, 338850)


def test_single_class_and_single_rows():
    emb, starts, H = pl.lattice_classes([70], seed=13, flips=32)
    got, _ = run_hist(emb, starts, 0, [0], [21])
    gen, imp = vo.lattice_keys(H, starts)
    assert len(imp) == 0 and got[0, 1].sum() == 0
    assert_same_words(got, vo.histogram(gen, imp, [0], [21]))
    emb, starts, H = pl.lattice_classes([1, 1, 1], seed=14, flips=32)
    got, _ = run_hist(emb, starts, 0, [0], [21])
    assert_same_words(got, vo.histogram(*vo.lattice_keys(H, starts), [0], [21]))
    assert got[0, 0].sum() == 0 and got[0, 1, B + 1] == 3


# ---- the curve against the oracle, both metrics ---------------------------------------------------------------------------------------
def assert_curve(curve, gen, imp, fars=FARS):
    got = curve.tar_at_far(fars)
    want = [vo.tar_at_far(gen, imp, f) for f in fars]
    for g, w in zip(got, want):
        assert np.float32(g["threshold"]).tobytes() == np.float32(w["threshold"]).tobytes() and g == w, (g, w)
    assert curve.eer() == vo.eer(gen, imp)
    keys, ta, fa = curve.roc_counts()
    assert (ta, fa) == vo.roc_at(gen, imp, keys) and len(keys) > 7 * B          # metric 1: no edge above pi
    far, tar, thr = curve.roc()
    assert np.array_equal(thr.view(np.uint32), np.array(keys, np.uint32)) and far[-1] == 1.0 == tar[-1]
    auc, auc_lo, auc_hi = curve.auc()
    assert auc_lo <= float(vo.auc(gen, imp)) <= auc_hi and auc_lo <= auc <= auc_hi
    assert curve.nrof_passes <= 4 and (curve.nrof_genuine, curve.nrof_impostor) == (len(gen), len(imp))
    return got


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("sizes,E", POOLS, ids=POOL_IDS)
def test_curve_equals_the_oracle_on_the_device_bits(sizes, E, metric):
    emb, _, labels, chain = random_pool(tuple(sizes), E)
    gen, imp = device_keys(tuple(sizes), E, metric)
    assert_curve(st.VerificationCurve(emb, labels, metric=metric, device=DEV), gen, imp)
    if metric == 0:                                                      # and the device's bits are the host chain's
        assert np.array_equal(gen, chain[0]) and np.array_equal(imp, chain[1])


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("sizes,E", POOLS[:2], ids=POOL_IDS[:2])
def test_threshold_means_the_same_to_the_gallery(sizes, E, metric):
    from facenet_amd.recognize import Gallery
    emb, _, labels, _ = random_pool(tuple(sizes), E)
    gallery = Gallery(emb, labels, metric=metric, device=DEV)
    records = st.VerificationCurve(emb, labels, metric=metric, device=DEV).tar_at_far(FARS)
    assert np.isinf(records[-1]["threshold"]) and sum(np.isfinite(r["threshold"]) for r in records) == len(FARS) - 1
    for r in records[:-1]:
        offsets, rows, _ = gallery.neighbours(np.float32(r["threshold"]))
        offsets, rows = offsets.cpu().numpy(), rows.cpu().numpy()
        same = labels[np.repeat(np.arange(len(labels)), np.diff(offsets))] == labels[rows]
        assert int(np.count_nonzero(~same)) == 2 * r["false_accepts"], r
        assert int(np.count_nonzero(same)) == 2 * r["true_accepts"], r


# ---- invariance and hygiene -----------------------------------------------------------------------------------------------------------
def test_two_runs_give_the_same_words():
    emb, starts, _, (gen, imp) = random_pool(tuple(POOLS[0][0]), POOLS[0][1])
    lo, shift = mixed_windows(gen, imp)
    first, _ = run_hist(emb, starts, 1, lo, shift)
    again, _ = run_hist(emb, starts, 1, lo, shift)
    assert first.tobytes() == again.tobytes() and first[6, 1, :B].sum() == len(imp)


def test_row_order_does_not_matter():
    from tests import validation_folds_oracle as fo
    sizes, E = POOLS[0]
    shuffled, shuffled_labels = fo.pool(sizes, E, seed=len(sizes))       # the same rows before pair_lattice.sorted_pool sorts them
    emb, _, labels, _ = random_pool(tuple(sizes), E)
    a = st.VerificationCurve(emb, labels, device=DEV)
    b = st.VerificationCurve(torch.from_numpy(shuffled), shuffled_labels, device=DEV)
    assert a.tar_at_far(FARS) == b.tar_at_far(FARS) and a.eer() == b.eer() and a.roc_counts() == b.roc_counts()


def test_odd_embedding_length_is_padded():
    sizes, E = pl.RANDOM_POOLS[4]
    assert E == 67
    emb, _, labels = pl.sorted_pool(list(sizes), E)
    a = st.VerificationCurve(emb, labels, device=DEV)
    assert a._emb.shape[1] == 68
    b = st.VerificationCurve(np.pad(emb, ((0, 0), (0, 1))), labels, device=DEV)
    assert a.tar_at_far(FARS) == b.tar_at_far(FARS) and a.eer() == b.eer() and a.roc_counts() == b.roc_counts()
    starts = np.concatenate([[0], np.cumsum(sizes)])
    assert_curve(a, *gallery_keys(np.pad(emb, ((0, 0), (0, 1))), starts, labels, 0))


def test_argument_errors():
    lib = _lib.load()
    emb, starts, _, _ = random_pool(tuple(POOLS[0][0]), POOLS[0][1])
    e, s = _dev(emb, np.float32), _dev(starts, np.int32)
    out = torch.zeros(9 * 2 * (B + 2), dtype=torch.int64, device=DEV)
    C, E = len(starts) - 1, emb.shape[1]

    def message(**kw):
        a = dict(emb_ptr=e.data_ptr(), cls_ptr=s.data_ptr(), C=C, E=E, metric=0, lo=[0], shift=[21], R=1, out_ptr=out.data_ptr(), rng_ptr=None)
        a.update(kw)
        assert launch(**a) == -1
        return lib.fn_last_error().decode()

    assert "number of windows must be in [1, 8] (R 0)" in message(R=0, lo=[], shift=[])
    assert "number of windows must be in [1, 8] (R 9)" in message(R=9, lo=[0] * 9, shift=[21] * 9)
    assert "shift must be in [0, 22] (window 1: shift 23)" in message(R=2, lo=[0, 0], shift=[3, 23])
    assert "shift must be in [0, 22] (window 0: shift -1)" in message(shift=[-1])
    assert "multiple of 4 in [4, 512] (E 6)" in message(E=6)
    assert "multiple of 4 in [4, 512] (E 516)" in message(E=516)
    assert "16-byte aligned" in message(emb_ptr=e.data_ptr() + 4)
    assert "16-byte aligned" in message(out_ptr=out.data_ptr() + 8)
    assert "Undefined similarity metric 2" in message(metric=2)
    torch.cuda.synchronize()
    assert int(out.abs().sum()) == 0                                     # no refused call launched anything
    with pytest.raises(ValueError, match="multiple of 4 in"):
        st.VerificationCurve(np.pad(emb, ((0, 0), (0, 516 - E))), np.repeat(np.arange(C), np.diff(starts)), device=DEV).eer()


def test_rows_off_the_unit_sphere_are_refused():
    emb, _, labels, _ = random_pool(tuple(POOLS[0][0]), POOLS[0][1])
    twice = np.concatenate([emb, emb[:1]]), np.concatenate([labels, labels[:1]])       # a duplicate: its dot is the squared norm
    assert st.VerificationCurve(*twice, device=DEV).tar_at_far([0.01])[0]["false_accepts"] >= 0
    with pytest.raises(ValueError, match="embeddings must be normalized to 1"):
        st.VerificationCurve(1.01 * twice[0], twice[1], device=DEV).tar_at_far([0.01])
    with pytest.raises(ValueError, match="genuine and impostor pairs"):
        st.VerificationCurve(emb[:5], [0, 1, 2, 3, 4], device=DEV)


# ---- the app --------------------------------------------------------------------------------------------------------------------------
class _PixelModel:
    """In place of the network: the first 64 pixel values of an image, centred and normalised.  The app's wiring is under test."""

    def __init__(self, config):
        self.config = config

    def evaluate(self, images):
        x = torch.as_tensor(images).cpu().reshape(len(images), -1)[:, :64].to(torch.float32) - 127.5
        return torch.nn.functional.normalize(x, dim=1)


def test_validate_app_appends_the_curve(tmp_path, monkeypatch):
    from PIL import Image
    import facenet_amd.api
    from facenet_amd.apps.validate import load_options, validate
    monkeypatch.setattr(facenet_amd.api, "FaceNet", _PixelModel)
    rng = np.random.default_rng(0)
    data = tmp_path / "faces"
    for c, n in enumerate((7, 8)):
        (data / f"id_{c:03d}").mkdir(parents=True)
        for i in range(n):
            Image.fromarray(rng.integers(0, 256, (160, 160, 3), dtype=np.uint8)).save(data / f"id_{c:03d}" / f"img_{i:03d}.png")
    texts, reports = [], []
    for k, extra in enumerate(({}, {"far_targets": [0.01]})):
        overrides = {"batch_size": 8, "dataset": {"path": str(data)}, "model": {"path": None},
                     "validate": dict({"nrof_folds": 3}, **extra), "file": str(tmp_path / f"report{k}.txt")}
        lines = []
        reports.append(validate(load_options(overrides=overrides), log=lambda s: lines.append(str(s))))
        texts.append(((tmp_path / f"report{k}.txt").read_text(), lines))
    (plain, plain_log), (full, full_log) = texts
    assert reports[0].curve is None and "VerificationCurve" not in plain and not any("VerificationCurve" in l for l in plain_log)
    curve = reports[1].curve
    block = 64 * "-" + "\n" + str(curve)
    assert isinstance(curve, st.VerificationCurve) and full.count(block) == 1 and str(curve) in full_log
    assert "TAR @ FAR = 0.01\n" in block and (curve.nrof_genuine, curve.nrof_impostor) == (21 + 28, 56)
    # without the block the file has the lines it has without the key (dates and times apart)
    strip = lambda t: [l for l in t.split("\n") if not l.startswith(("FaceToFaceValidation 20", "elapsed time: ", str(tmp_path)))]
    assert strip(full.replace(block, "")) == strip(plain)
    assert full.index(block) > full.index("FalseAlarmRate(FAR = 0.001)") and full.split("\n")[-2].startswith("elapsed time: ")
    # the class by hand
    from facenet_amd import dataset
    opt = load_options(overrides=overrides)
    batches = dataset.Database(opt.dataset).tf_dataset_api(loader=dataset.ImageLoader(config=opt.image), batch_size=8)
    model = _PixelModel(None)
    seen = [(model.evaluate(x).numpy(), np.asarray(l.cpu() if torch.is_tensor(l) else l)) for x, l in batches]
    emb, labels = np.concatenate([e for e, _ in seen]), np.concatenate([l for _, l in seen])
    by_hand = st.VerificationCurve(emb, labels, device=DEV)
    assert by_hand.tar_at_far([0.01]) == curve.tar_at_far([0.01]) and by_hand.eer() == curve.eer() and by_hand.auc() == curve.auc()


def test_validate_callback_appends_the_curve(tmp_path):
    from facenet_amd import callbacks
    from facenet_amd.config import Config
    emb, _, labels, _ = random_pool(tuple(POOLS[0][0]), POOLS[0][1])
    data = [(emb[:50], labels[:50]), (emb[50:], labels[50:])]              # the "images" are the embeddings: the model is the identity

    class Model:
        path = tmp_path / "run"

        def __call__(self, images):
            return images

    class Report:
        dict = {}

        def __init__(self, *a):
            pass

        def __repr__(self):
            return "stub report\n"

        def write_report(self, file):
            with open(file, "at") as f:
                f.write(str(self))

    lines = []
    cb = callbacks.ValidateCallback(Model(), data, 1, 1, Config({"validate": {"metric": 1, "far_targets": [1e-3, 0.1]}}),
                                    log=lambda s: lines.append(str(s)), statistic=Report)
    curve = cb.on_epoch_end(0).curve
    assert isinstance(curve, st.VerificationCurve) and curve.metric == 1
    assert (tmp_path / "run" / "report.txt").read_text() == "stub report\n" + 64 * "-" + "\n" + str(curve) and str(curve) in lines
    by_hand = st.VerificationCurve(emb, labels, metric=1, device=DEV)
    assert by_hand.tar_at_far([1e-3, 0.1]) == curve.tar_at_far([1e-3, 0.1]) and by_hand.eer() == curve.eer()
    assert str(curve).count("TAR @ FAR = ") == 2
