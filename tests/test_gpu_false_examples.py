"""fn_false_pairs and FalseExamples on the device against tests/false_examples_oracle.py: the rows of every
pick, the order of the picks and, at metric 0, every bit of the distances.  The lattice pools are full of exact ties, so the
tie-break (first in the row-major order of the reference's matrices) decides most picks."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from facenet_amd import _lib, utils
from facenet_amd import statistics as st
from tests import false_examples_oracle as fe
from tests import pair_lattice as pl

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = [5, 1, 9, 33, 2, 40, 7]
MAXES = [(10, 2), (3, 5)]
GUARD = 8
FILL = -77


def class_of(starts):
    return np.repeat(np.arange(len(starts) - 1), np.diff(starts))


def run(emb, starts, threshold, **kw):
    """FalseExamples over rows that are sorted by class already: its indices are the oracle's rows."""
    return st.FalseExamples(emb, class_of(starts), threshold, device=DEV, **kw)


def assert_same(got, want, exact=True, tol=0.0):
    """got: FalseExamples; want: the oracle's (false negatives, false positives).  Rows and order always; the distances bit for
    bit (exact) or within tol."""
    for name, have, lst in (("false negatives", got.false_negatives, want[0]), ("false positives", got.false_positives, want[1])):
        assert [(a, b) for _, a, b in have] == [(a, b) for _, a, b in lst], name
        assert all(type(d) is float and type(a) is int and type(b) is int for d, a, b in have)
        if exact:
            bad = [(h, w) for h, w in zip(have, lst) if np.float32(h[0]).tobytes() != np.float32(w[0]).tobytes()]
            assert not bad, (name, bad[:4])
        else:
            assert all(abs(h[0] - float(w[0])) <= tol for h, w in zip(have, lst)), name
    assert (got.nrof_false_negatives, got.nrof_false_positives) == (len(want[0]), len(want[1]))


# ---- 1. lattice pools -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def lattice_pool(E_pad):
    return pl.lattice_classes(SIZES, seed=31, flips=32, E_pad=E_pad)


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("E_pad", [0, 4])
def test_lattice_pools(E_pad, metric):
    emb, starts, H = lattice_pool(E_pad)
    D = fe.lattice_distances(H, metric)
    thresholds = pl.lattice_thresholds(metric)
    some = 0
    for t in (thresholds[8], thresholds[32], thresholds[56]):
        for max_fneg, max_fpos in MAXES:
            want = fe.false_pairs(D, starts, t, max_fneg, max_fpos)
            got = run(emb, starts, t, metric=metric, max_fneg=max_fneg, max_fpos=max_fpos)
            assert_same(got, want, exact=metric == 0, tol=pl.ACOS_EPS)
            some += len(want[0]) > 0 and len(want[1]) > 0
    assert some >= 2                                         # both kinds at once, at more than one setting


# ---- 2. tile edges --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def edge_pool():
    """1, 2 and 3 super-tiles in each direction and a one-row class.  Planted: the last row of the 130-row class duplicates the
    last row of the 65-row class (d = 0 in the last row and last column of that pair of classes) and its last but one row is its
    last row negated (d = 4 at the last pair of the class)."""
    sizes = [63, 64, 65, 130, 1]
    emb, starts, _ = pl.lattice_classes(sizes, seed=32, flips=8, E_pad=16, E0=16)
    emb = emb.copy()
    emb[starts[4] - 1] = emb[starts[3] - 1]
    emb[starts[4] - 2] = -emb[starts[4] - 1]
    return emb, starts, fe.chain_distances(emb)


@pytest.mark.parametrize("threshold", [0.25, 1.0, 2.0, 3.75])
def test_tile_edges(threshold):
    emb, starts, D = edge_pool()
    assert emb.shape == (323, 32)
    last65, last130 = int(starts[3] - 1), int(starts[4] - 1)
    assert D[last65, last130] == 0.0 and D[last130 - 1, last130] == 4.0
    for max_fneg, max_fpos in ((10, 2), (64, 64)):
        want = fe.false_pairs(D, starts, threshold, max_fneg, max_fpos)
        assert_same(run(emb, starts, threshold, max_fneg=max_fneg, max_fpos=max_fpos), want)
    planted = [(a, b) for _, a, b in want[0] + want[1]]
    assert (last65, last130) in planted and (last130 - 1, last130) in planted          # at 64 picks both planted pairs are reached


# ---- 3. grid stride -------------------------------------------------------------------------------------------------------------------
def test_many_class_pairs_per_workgroup():
    sizes, emb, starts, H = pl.many_class_pool()
    D = fe.lattice_distances(H, 0, E0=16)
    want = fe.false_pairs(D, starts, 1.0)
    assert len(want[0]) > 100 and len(want[1]) > 1000
    got = run(emb, starts, 1.0)
    assert_same(got, want)


# ---- 4. random rows -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sizes,E", pl.RANDOM_POOLS, ids=["7-classes-E128", "20x3-E512", "70-45-E96", "150-3-40-E100", "5-classes-E67"])
def test_random_rows(sizes, E):
    emb, starts, _ = pl.sorted_pool(list(sizes), E)
    D = fe.chain_distances(emb)
    seen = [0, 0]
    for t in (0.8, 1.3, 2.0):                                # the classes are separable: inside the genuine range, between, inside the impostors'
        want = fe.false_pairs(D, starts, t)
        got = run(emb, starts, t)
        assert_same(got, want)
        seen = [seen[0] + len(want[0]), seen[1] + len(want[1])]
    assert min(seen) > 0
    if E % 4:                                                # the host pads; the padded table gives the same records
        padded, plain = run(np.pad(emb, ((0, 0), (0, 4 - E % 4))), starts, 0.8), run(emb, starts, 0.8)
        assert (padded.false_negatives, padded.false_positives) == (plain.false_negatives, plain.false_positives)


# ---- 5. orientation -------------------------------------------------------------------------------------------------------------------
def test_orientation_of_the_tie_break():
    """a = (x, y) and b = (y, x): d(a0, b1) = d(a1, b0) = 0.  The reference's rows are the LOWER class: (a0, b1) comes first."""
    emb, _, _ = lattice_pool(0)
    x, y = emb[0], emb[5]
    assert not np.array_equal(x, y)
    rows = np.stack([y, x, x, y])                            # b0, b1, a0, a1: the higher label first
    got = st.FalseExamples(rows, [7, 7, 3, 3], 1.0, max_fpos=2, device=DEV)
    assert got.false_positives == [(0.0, 2, 1), (0.0, 3, 0)]
    D = fe.chain_distances(np.stack([x, y, y, x]))           # sorted by label: a0, a1, b0, b1
    assert [(a, b) for _, a, b in fe.false_positives(D, [0, 2, 4], 1.0)] == [(0, 3), (1, 2)]


# ---- 6. ceilings and strictness ---------------------------------------------------------------------------------------------------------
def test_ceilings_and_strictness():
    emb, starts, _ = lattice_pool(4)
    emb = emb.copy()
    emb[starts[2] + 4] = emb[starts[0]]                      # a duplicate across classes: d = +0
    D = fe.chain_distances(emb)
    cls, sizes = class_of(starts), np.diff(starts)
    for max_fneg, max_fpos in MAXES:
        kw = dict(max_fneg=max_fneg, max_fpos=max_fpos)
        # above every distance: every pair of classes yields its ceiling, and no false negative
        got = run(emb, starts, 5.0, **kw)
        per_pair = {}
        for _, a, b in got.false_positives:
            per_pair[(cls[a], cls[b])] = per_pair.get((cls[a], cls[b]), 0) + 1
        assert per_pair == {(a, b): min(max_fpos, sizes[a], sizes[b]) for a in range(len(sizes)) for b in range(a + 1, len(sizes))}
        assert got.false_negatives == []
        assert_same(got, fe.false_pairs(D, starts, 5.0, **kw))
        # below every distance: every class yields its ceiling, and no false positive
        got = run(emb, starts, -1.0, **kw)
        assert np.array_equal(np.bincount([cls[a] for _, a, _ in got.false_negatives], minlength=len(sizes)), np.minimum(max_fneg, sizes // 2))
        assert got.false_positives == []
        assert_same(got, fe.false_pairs(D, starts, -1.0, **kw))
        # strict: d = +0 is not < 0.0 and d = 4.0 is not > 4.0
        got = run(emb, starts, 0.0, **kw)
        assert D[starts[0], starts[2] + 4] == 0.0 and got.false_positives == [] and got.nrof_false_negatives > 0
        assert_same(got, fe.false_pairs(D, starts, 0.0, **kw))
        got = run(emb, starts, 4.0, **kw)
        assert D.max() == 4.0 and got.false_negatives == [] and got.nrof_false_positives > 0
        assert_same(got, fe.false_pairs(D, starts, 4.0, **kw))
    for t in (5.0, -1.0, 2.0):
        want = fe.false_pairs(D, starts, t)
        got = run(emb, starts, t, max_fneg=0)
        assert got.false_negatives == [] and [(a, b) for _, a, b in got.false_positives] == [(a, b) for _, a, b in want[1]]
        got = run(emb, starts, t, max_fpos=0)
        assert got.false_positives == [] and [(a, b) for _, a, b in got.false_negatives] == [(a, b) for _, a, b in want[0]]
        got = run(emb, starts, t, max_fneg=0, max_fpos=0)
        assert got.false_negatives == [] and got.false_positives == []


# ---- 7. capacity ----------------------------------------------------------------------------------------------------------------------
def raw(emb, starts, threshold, capacity, max_fneg=10, max_fpos=2, metric=0, records=True):
    """One call of the entry itself -> (count [2], records int32 [capacity, 4]); asserts that the guard rows behind `records` and
    the guard words behind `count` and `range` are untouched."""
    lib = _lib.load()
    e = torch.from_numpy(np.ascontiguousarray(emb, np.float32)).to(DEV)
    s = torch.from_numpy(np.ascontiguousarray(starts, np.int32)).to(DEV)
    rec = torch.full((capacity + GUARD, 4), FILL, dtype=torch.int32, device=DEV)
    count = torch.full((2 + GUARD,), FILL, dtype=torch.int64, device=DEV)
    count[:2] = 0                                            # the caller zeroes count
    rng = torch.full((2 + GUARD,), FILL, dtype=torch.int32, device=DEV)
    rc = lib.fn_false_pairs(e.data_ptr(), s.data_ptr(), len(starts) - 1, emb.shape[1], metric, ctypes.c_float(threshold), max_fneg, max_fpos,
                            rec.data_ptr() if records else None, capacity if records else 0, count.data_ptr(), rng.data_ptr(),
                            torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.fn_last_error()
    torch.cuda.synchronize()
    rec, count, rng = rec.cpu().numpy(), count.cpu().numpy(), rng.cpu().tolist()
    assert (rec[capacity:] == FILL).all() and (count[2:] == FILL).all() and rng[2:] == [FILL] * GUARD
    if not records:
        assert (rec == FILL).all()
    return count[:2].tolist(), rec[:capacity], (st._decode_ord(rng[0]), st._decode_ord(rng[1]))


def as_records(pairs, cls):
    """The oracle's list -> the set of the entry's records (row1, row2, bits of d, pick index within its class or pair)."""
    out, pick, last = set(), 0, None
    for d, a, b in pairs:
        pick = pick + 1 if last == (cls[a], cls[b]) else 0
        last = (cls[a], cls[b])
        out.add((a, b, int(np.float32(d).view(np.int32)), pick))
    return out


def test_capacity_and_the_raw_entry():
    emb, starts, H = lattice_pool(4)
    D = fe.lattice_distances(H, 0)
    want = fe.false_pairs(D, starts, 2.0)
    nneg, npos = len(want[0]), len(want[1])
    assert nneg > 12 and npos > 12
    want_neg, want_pos = as_records(want[0], class_of(starts)), as_records(want[1], class_of(starts))
    records = want_neg | want_pos
    assert len(records) == nneg + npos
    # room for all: the front holds the false negatives, the back the false positives
    count, rec, rng = raw(emb, starts, 2.0, nneg + npos + 3)
    assert count == [nneg, npos] and rng == pl.want_range(pl.exact_dots(H), starts)
    assert {tuple(int(v) for v in r) for r in rec[:nneg]} == want_neg
    assert {tuple(int(v) for v in r) for r in rec[3 + nneg:]} == want_pos and (rec[nneg:nneg + 3] == FILL).all()
    # too little room: the counts are the true ones, only `capacity` rows are written and each holds a record
    count, rec, _ = raw(emb, starts, 2.0, 12)
    assert count == [nneg, npos] and {tuple(int(v) for v in r) for r in rec} <= records
    count, rec, _ = raw(emb, starts, 2.0, 0, records=False)
    assert count == [nneg, npos]
    # the class names both numbers
    with pytest.raises(ValueError, match=r"found {} pairs \({} false negatives, {} false positives\), more than max_records = {}:".format(
            nneg + npos, nneg, npos, nneg + npos - 1)):
        run(emb, starts, 2.0, max_records=nneg + npos - 1)
    assert_same(run(emb, starts, 2.0, max_records=nneg + npos), want)
    # the default buffer is the true upper bound
    assert_same(run(emb, starts, 5.0, max_fneg=64, max_fpos=64), fe.false_pairs(D, starts, 5.0, 64, 64))


# ---- 8. the caller's order ------------------------------------------------------------------------------------------------------------
def test_callers_order_and_files():
    from tests import validation_folds_oracle as fo
    sizes, E = pl.RANDOM_POOLS[2]
    emb, labels = fo.pool(sizes, E, seed=len(sizes))         # shuffled
    assert np.any(np.diff(labels) < 0)
    order = np.argsort(labels, kind="stable")
    starts = np.concatenate([[0], np.cumsum(np.unique(labels, return_counts=True)[1])])
    want = fe.false_pairs(fe.chain_distances(emb[order]), starts, 1.3)
    files = ["/data/id_{:03d}/img_{:04d}.jpg".format(l, i) for i, l in enumerate(labels)]
    got = st.FalseExamples(torch.from_numpy(emb), labels, 1.3, files=files, device=DEV)
    for have, lst in ((got.false_negatives, want[0]), (got.false_positives, want[1])):
        assert len(lst) > 0 and [(np.float32(d).tobytes(), a, b) for d, a, b in have] == [(d.tobytes(), int(order[a]), int(order[b])) for d, a, b in lst]
    assert all(labels[a] == labels[b] for _, a, b in got.false_negatives) and all(labels[a] < labels[b] for _, a, b in got.false_positives)
    again = st.FalseExamples(emb, labels, 1.3, files=files, device=DEV)
    assert (again.false_negatives, again.false_positives) == (got.false_negatives, got.false_positives) and repr(again) == repr(got)
    d, a, b = min(got.false_positives, key=lambda r: r[0])
    text = repr(got)
    assert text.startswith("FalseExamples\nmetric: 0\nthreshold: 1.30000\n\nfalse negatives: {} (at most 10 per class)\n".format(len(want[0])))
    assert "Nearest false positive: {:2.5f} {} & {}\n".format(d, utils.file2text(files[a]), utils.file2text(files[b])) in text
    assert "Farthest false negative: " in text and "id_{:03d}/img_{:04d}".format(labels[a], a) in text
    with pytest.raises(ValueError, match="needs the files"):
        st.FalseExamples(emb, labels, 1.3, device=DEV).write_false_pairs("a", "b")


# ---- 9. the normalisation check ---------------------------------------------------------------------------------------------------------
def test_rows_off_the_unit_sphere_are_refused():
    emb, starts, _ = pl.sorted_pool(*pl.RANDOM_POOLS[0])
    labels = class_of(starts)
    twice = np.concatenate([emb, emb[:1]]), np.concatenate([labels, labels[:1]])       # a duplicate: its dot is the squared norm
    assert st.FalseExamples(*twice, 1.25, device=DEV).nrof_false_positives >= 0
    with pytest.raises(ValueError, match="embeddings must be normalized to 1"):
        st.FalseExamples(1.01 * twice[0], twice[1], 1.25, device=DEV)


# ---- 10. the app ----------------------------------------------------------------------------------------------------------------------
class _PixelModel:
    """In place of the network: the first 64 pixel values of an image, centred and normalised.  The app's wiring is under test."""

    def __init__(self, config):
        self.config = config

    def evaluate(self, images):
        x = torch.as_tensor(images).cpu().reshape(len(images), -1)[:, :64].to(torch.float32) - 127.5
        return torch.nn.functional.normalize(x, dim=1)


def test_validate_app_appends_the_block_and_writes_the_pairs(tmp_path, monkeypatch):
    from PIL import Image
    import facenet_amd.api
    from facenet_amd import dataset
    from facenet_amd.apps.validate import load_options, validate
    monkeypatch.setattr(facenet_amd.api, "FaceNet", _PixelModel)
    rng = np.random.default_rng(0)
    data = tmp_path / "faces"
    for c, n in enumerate((7, 8)):
        (data / f"id_{c:03d}").mkdir(parents=True)
        for i in range(n):
            Image.fromarray(rng.integers(0, 256, (160, 160, 3), dtype=np.uint8)).save(data / f"id_{c:03d}" / f"img_{i:03d}.png")
    texts, reports = [], []
    for k, extra in enumerate(({}, {"false_examples": {"threshold": 2.0, "max_fneg": 3, "max_fpos": 4}})):
        overrides = {"batch_size": 8, "dataset": {"path": str(data)}, "model": {"path": None},
                     "validate": dict({"nrof_folds": 3}, **extra), "file": str(tmp_path / f"run{k}" / "report.txt")}
        lines = []
        reports.append(validate(load_options(overrides=overrides), log=lambda s: lines.append(str(s))))
        texts.append(((tmp_path / f"run{k}" / "report.txt").read_text(), lines))
    (plain, plain_log), (full, full_log) = texts
    assert reports[0].false_examples is None and "FalseExamples" not in plain and not any("FalseExamples" in l for l in plain_log)
    assert sorted(f.name for f in (tmp_path / "run0").iterdir()) == ["report.txt"]
    found = reports[1].false_examples
    block = 64 * "-" + "\n" + str(found)
    assert isinstance(found, st.FalseExamples) and full.count(block) == 1 and str(found) in full_log and full.count("FalseExamples\n") == 1
    strip = lambda t: [l for l in t.split("\n") if not l.startswith(("FaceToFaceValidation 20", "elapsed time: ", str(tmp_path)))]
    assert strip(full.replace(block, "")) == strip(plain)
    assert full.index(block) > full.index("FalseAlarmRate(FAR = 0.001)") and full.split("\n")[-2].startswith("elapsed time: ")
    # the oracle over the embeddings computed by hand: the database's order is the evaluation's
    opt = load_options(overrides=overrides)
    dbase = dataset.Database(opt.dataset)
    batches = dbase.tf_dataset_api(loader=dataset.ImageLoader(config=opt.image), batch_size=8)
    model = _PixelModel(None)
    seen = [(model.evaluate(x).numpy(), np.asarray(l.cpu() if torch.is_tensor(l) else l)) for x, l in batches]
    emb, labels = np.concatenate([e for e, _ in seen]), np.concatenate([l for _, l in seen])
    assert np.all(np.diff(labels) >= 0) and len(dbase.files) == 15
    want = fe.false_pairs(fe.chain_distances(emb), [0, 7, 15], 2.0, 3, 4)
    assert len(want[0]) > 0 and len(want[1]) > 0
    for sub, lst in (("false_negatives", want[0]), ("false_positives", want[1])):
        names = sorted(utils.generate_filename(tmp_path / "run1" / sub, float(d), dbase.files[a], dbase.files[b]) for d, a, b in lst)
        assert sorted(str(f) for f in (tmp_path / "run1" / sub).iterdir()) == names and len(set(names)) == len(lst)
    width, height = Image.open(names[0]).size
    assert (width, height) == (320, 160)
    by_hand = st.FalseExamples(emb, labels, 2.0, files=dbase.files, max_fneg=3, max_fpos=4, device=DEV)
    assert_same(by_hand, want)
    assert (by_hand.false_negatives, by_hand.false_positives) == (found.false_negatives, found.false_positives) and str(by_hand) == str(found)
