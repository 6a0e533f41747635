"""The host side of the false examples: the NumPy oracle against cases worked by hand, the file names and
pictures of facenet_amd.utils, and the argument rules of fn_false_pairs, each refused before any launch."""
import ctypes
from pathlib import Path

import numpy as np
import pytest

from facenet_amd import utils
from tests import false_examples_oracle as fe

STARTS = np.array([0, 4, 7, 9])          # classes A = rows 0..3, B = 4..6, C = 7..8


def matrix(d23=3.0):
    """A symmetric 9 x 9 table of distances; every entry not listed is 2.0 between classes and 0.25 within one."""
    D = np.full((9, 9), 2.0, np.float32)
    for a, b in zip(STARTS[:-1], STARTS[1:]):
        D[a:b, a:b] = 0.25
    listed = {(0, 1): 3.0, (2, 3): d23, (0, 2): 2.5, (0, 3): 1.0, (1, 2): 2.0, (1, 3): 0.5,            # within A
              (4, 5): 1.0, (4, 6): 0.2, (5, 6): 0.3,                                                    # within B
              (7, 8): 1.5,                                                                              # within C
              (0, 4): 0.5, (1, 5): 0.5, (0, 5): 0.6, (1, 4): 0.7, (2, 6): 1.0,                          # A x B
              (0, 7): 0.125, (0, 8): 0.25, (1, 7): 0.375, (1, 8): 0.875}                                # A x C
    for (i, k), d in listed.items():
        D[i, k] = D[k, i] = d
    D[4:7, 7:9] = D[7:9, 4:7] = 0.5                                                                     # B x C: one value
    np.fill_diagonal(D, 0.0)
    return D


def pairs(records):
    return [(r1, r2) for _, r1, r2 in records]


def test_false_negatives_by_hand():
    D = matrix()
    got = fe.false_negatives(D, STARTS, 1.0)
    # A: (0, 1) and (2, 3) tie at 3.0 and the first in row-major order goes first; B: 1.0 is not > 1.0; C: its one pair
    assert got == [(np.float32(3.0), 0, 1), (np.float32(3.0), 2, 3), (np.float32(1.5), 7, 8)]
    assert all(type(d) is np.float32 for d, _, _ in got)
    # both images of a pick leave the class: with (2, 3) below the threshold nothing follows (0, 1), although (0, 2) = 2.5 and
    # (1, 2) = 2.0 are above it
    assert pairs(fe.false_negatives(matrix(d23=0.875), STARTS, 1.0)) == [(0, 1), (7, 8)]
    # strictness: one ulp below 1.0 admits B's (4, 5) and A's (0, 3) stays behind its excluded rows
    below = np.nextafter(np.float32(1.0), np.float32(0))
    assert pairs(fe.false_negatives(D, STARTS, below)) == [(0, 1), (2, 3), (4, 5), (7, 8)]
    # ceilings: min(max_fneg, n // 2) = 2, 1, 1 at a threshold every pair exceeds; max_fneg = 1 and 0 cut further
    everything = fe.false_negatives(D, STARTS, -1.0, max_fneg=10)
    assert pairs(everything) == [(0, 1), (2, 3), (4, 5), (7, 8)] and len(everything) == sum(min(10, n // 2) for n in (4, 3, 2))
    assert pairs(fe.false_negatives(D, STARTS, -1.0, max_fneg=1)) == [(0, 1), (4, 5), (7, 8)]
    assert fe.false_negatives(D, STARTS, -1.0, max_fneg=0) == [] and fe.false_negatives(D, STARTS, 4.0) == []


def test_false_positives_by_hand():
    D = matrix()
    got = fe.false_positives(D, STARTS, 1.0)
    # A x B: (0, 4) and (1, 5) tie at 0.5, row-major first; A x C: image 0 is free again (exclusion is per pair of classes), then
    # (0, 8) = 0.25 is behind row 0 and (1, 7) = 0.375 behind column 7: the second pick is (1, 8); B x C: all ties
    assert got == [(np.float32(0.5), 0, 4), (np.float32(0.5), 1, 5), (np.float32(0.125), 0, 7), (np.float32(0.875), 1, 8),
                   (np.float32(0.5), 4, 7), (np.float32(0.5), 5, 8)]
    # strictness: (2, 6) = 1.0 is not < 1.0, so a third pick of A x B finds nothing; one ulp above it does
    above = np.nextafter(np.float32(1.0), np.float32(2))
    assert pairs(fe.false_positives(D, STARTS, 1.0, max_fpos=3))[:3] == [(0, 4), (1, 5), (0, 7)]
    assert pairs(fe.false_positives(D, STARTS, above, max_fpos=3))[:3] == [(0, 4), (1, 5), (2, 6)]
    # ceilings: min(max_fpos, na, nb) = 3, 2, 2 at a threshold above every distance
    everything = fe.false_positives(D, STARTS, 5.0, max_fpos=5)
    assert [sum(1 for _, r1, r2 in everything if r1 < 4 and 4 <= r2 < 7), sum(1 for _, r1, r2 in everything if r1 < 4 and r2 >= 7),
            sum(1 for _, r1, r2 in everything if r1 >= 4)] == [3, 2, 2]
    assert len({r1 for _, r1, r2 in everything if r2 >= 7 and r1 < 4}) == 2          # a row and a column are used once
    assert len(fe.false_positives(D, STARTS, 5.0, max_fpos=1)) == 3
    assert fe.false_positives(D, STARTS, 5.0, max_fpos=0) == [] and fe.false_positives(D, STARTS, 0.0) == []
    assert fe.records_bound([4, 3, 2], 10, 5) == 4 + 7 and fe.records_bound([4, 3, 2], 1, 1) == 3 + 3


def test_records_bound_counts_as_the_oracle_does():
    from facenet_amd.false_examples import records_bound
    rng = np.random.default_rng(0)
    for sizes in ([1], [2], [5, 1, 9, 33, 2, 40, 7], list(rng.integers(1, 9, 40))):
        for mx in ((10, 2), (3, 5), (0, 0), (64, 64), (1, 0)):
            assert records_bound(sizes, *mx) == fe.records_bound(sizes, *mx), (sizes, mx)


def test_file_names():
    assert utils.file2text("/data/faces/n000012/0007_01.jpg") == "n000012/0007_01"
    assert utils.file2text(Path("faces/id_001/img.000.png")) == "id_001/img.000"
    same = utils.generate_filename("/out/fneg", 1.23456, "/data/n000012/0007_01.jpg", "/data/n000012/0011_02.png")
    assert same == "/out/fneg/n000012|0007_01 & 0011_02 & 1.235.png"
    other = utils.generate_filename(Path("out"), 0.5, "/data/n000012/0007_01.jpg", "/data/n000345/0001_01.jpg")
    assert other == "out/n000012|0007_01 & n000345|0001_01 & 0.500.png"
    assert utils.generate_filename("d", 12.0, "a/x.png", "b/x.png") == "d/a|x & b|x & 12.000.png"


def test_concatenated_images(tmp_path):
    from PIL import Image
    rng = np.random.default_rng(1)
    h, w = 96, 80
    files, pixels = [], []
    for c, name in (("id_000", "left.png"), ("id_001", "right.png")):
        (tmp_path / c).mkdir()
        pixels.append(rng.integers(0, 256, (h, w, 3), dtype=np.uint8))
        files.append(tmp_path / c / name)
        Image.fromarray(pixels[-1]).save(files[-1])
    out = tmp_path / "pairs"
    out.mkdir()
    picture = utils.ConcatenateImages(files[0], files[1], 0.75)
    picture.save(out)
    assert [f.name for f in out.iterdir()] == ["id_000|left & id_001|right & 0.750.png"]
    got = np.array(Image.open(out / "id_000|left & id_001|right & 0.750.png"))
    assert got.shape == (h, 2 * w, 3)
    text = 48                                             # two lines of a 13-point font end well above this row
    assert np.array_equal(got[text:, :w], pixels[0][text:]) and np.array_equal(got[text:, w:], pixels[1][text:])
    before = np.concatenate(pixels, axis=1)[:text].astype(int)
    changed = (got[:text] != before).any(axis=2)                                           # thin strokes, blended into the pixels
    assert changed.sum() > 20 and (got[:text].astype(int) - before)[changed][:, 1].min() >= 0          # towards green


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------
def test_symbol_is_declared_and_exported():
    from facenet_amd import _lib
    header = (Path(__file__).resolve().parents[1] / "include" / "facenet_hip.h").read_text()
    assert "int fn_false_pairs(const float* emb, const int32_t* cls_start, int C, int E, int metric, float threshold" in header
    assert "fn_false_pairs" in _lib.EXPORTS
    lib = _lib.load()
    assert hasattr(lib, "fn_false_pairs") and lib.fn_abi_version() == 1


def test_argument_rules_are_refused_before_any_launch():
    """Host memory stands in for every buffer: a call that got as far as a launch would not return -1 with these messages."""
    from facenet_amd import _lib
    lib = _lib.load()
    emb = (ctypes.c_float * 64)()
    base = ctypes.addressof(emb) + (-ctypes.addressof(emb)) % 16
    cls = (ctypes.c_int32 * 3)(0, 1, 2)
    words = (ctypes.c_uint64 * 8)()

    def message(**kw):
        a = dict(emb=base, cls=ctypes.addressof(cls), C=2, E=4, metric=0, threshold=1.0, max_fneg=10, max_fpos=2, records=base + 32,
                 capacity=1, count=ctypes.addressof(words), rng=None)
        a.update(kw)
        rc = lib.fn_false_pairs(a["emb"], a["cls"], a["C"], a["E"], a["metric"], a["threshold"], a["max_fneg"], a["max_fpos"],
                                a["records"], a["capacity"], a["count"], a["rng"], None)
        assert rc == -1
        return lib.fn_last_error().decode()

    assert "false_pairs: the embedding length must be a multiple of 4 in [4, 512] (E 6)" in message(E=6)
    assert "multiple of 4 in [4, 512] (E 0)" in message(E=0)
    assert "multiple of 4 in [4, 512] (E 516)" in message(E=516)
    assert "Undefined similarity metric 2" in message(metric=2)
    assert "Undefined similarity metric -1" in message(metric=-1)
    assert "max_fneg must be in [0, 64] (max_fneg 65)" in message(max_fneg=65)
    assert "max_fneg must be in [0, 64] (max_fneg -1)" in message(max_fneg=-1)
    assert "max_fpos must be in [0, 64] (max_fpos 65)" in message(max_fpos=65)
    assert "max_fpos must be in [0, 64] (max_fpos -1)" in message(max_fpos=-1)
    assert "capacity must not be negative (capacity -1)" in message(capacity=-1)
    assert "records may be null only with capacity 0 (capacity 3)" in message(records=None, capacity=3)
    assert "bad arguments" in message(emb=None)
    assert "bad arguments" in message(cls=None)
    assert "bad arguments" in message(count=None)
    assert "bad arguments" in message(C=0)
    assert "too many classes (C 65536, at most 65535)" in message(C=65536)
    assert "16-byte aligned" in message(emb=base + 4)
    assert "16-byte aligned" in message(records=base + 40)
    assert "8-byte aligned" in message(count=ctypes.addressof(words) + 4)
    assert bytes(words) == bytes(64) and bytes(emb) == bytes(256)


def test_host_rules_are_refused_before_any_launch():
    from facenet_amd.false_examples import MAX_CLASS_ROWS, FalseExamples
    emb, labels = np.eye(4, dtype=np.float32), [0, 0, 1, 1]
    for kw, text in ((dict(metric=2), "Undefined similarity metric 2"), (dict(max_fneg=65), r"max_fneg must be an integer in \[0, 64\]"),
                     (dict(max_fpos=-1), r"max_fpos must be an integer in \[0, 64\]"), (dict(max_fpos=1.5), "max_fpos must be"),
                     (dict(threshold=float("nan")), "threshold must be a number"), (dict(files=["a/b.png"]), "one file per label"),
                     (dict(max_records=-1), "max_records must be")):
        args = dict(threshold=1.0, device="cpu")
        args.update(kw)
        with pytest.raises(ValueError, match=text):
            FalseExamples(emb, labels, **args)
    with pytest.raises(ValueError, match="a class has 65537 rows, more than the 65536"):
        FalseExamples(np.zeros((MAX_CLASS_ROWS + 2, 4), np.float32), [0] * (MAX_CLASS_ROWS + 1) + [1], 1.0, device="cpu")


def test_the_config_key_is_off_by_default(tmp_path):
    from facenet_amd import statistics as st
    from facenet_amd.apps.validate import DEFAULTS, load_options
    from facenet_amd.false_examples import FalseExamples, false_examples
    assert st.FalseExamples is FalseExamples and st.false_examples is false_examples
    assert "false_examples" not in DEFAULTS["validate"]
    opt = load_options(overrides={"model": {"path": str(tmp_path)}})
    assert false_examples(None, None, None, opt.validate, None) is None                 # nothing is looked at
    opt = load_options(overrides={"model": {"path": str(tmp_path)}, "validate": {"false_examples": None}})
    assert false_examples(None, None, None, opt.validate, None) is None
    opt = load_options(overrides={"model": {"path": str(tmp_path)}, "validate": {"false_examples": {"threshold": 1.25, "max_fpos": 3}}})
    assert opt.validate.false_examples.as_dict == {"threshold": 1.25, "max_fpos": 3} and opt.validate.nrof_folds == 10
    with pytest.raises(ValueError, match="max_fpos must be an integer in"):             # the section reaches the class
        false_examples(np.eye(2, dtype=np.float32), [0, 1], None, load_options(overrides={
            "model": {"path": str(tmp_path)}, "validate": {"false_examples": {"threshold": 1.0, "max_fpos": 99}}}).validate, 0.5, device="cpu")
