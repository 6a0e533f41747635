"""The call plumbing of the host wrappers (facenet_amd/_call.py) without a device: pointers, the embeddings
table, the workspace query against the library's own size rule, the `range` words and the integer check with its six texts."""
import numpy as np
import pytest
import torch

from facenet_amd import _call, _lib


def test_ptr_takes_none_and_an_element_offset():
    assert _call.ptr(None) is None and _call.ptr(None, 3) is None
    for dtype in (torch.float32, torch.int64, torch.uint8):
        t = torch.zeros(16, dtype=dtype)
        assert _call.ptr(t) == t.data_ptr()
        for off in (1, 5):
            assert _call.ptr(t, off) == t.data_ptr() + off * t.element_size()
    from facenet_amd import engine
    assert engine._ptr is _call.ptr                           # the name the plan builders import


def test_as_table_errors_and_realignment():
    with pytest.raises(ValueError, match=r"embeddings must be a 2-D \[n, E\] array, got shape \(8,\)"):
        _call.as_table(np.ones(8, np.float32), "cpu")
    with pytest.raises(ValueError, match="embedding length 6 must be a multiple of 4"):
        _call.as_table(np.ones((2, 6), np.float32), "cpu")
    base = torch.arange(2 * 8 + 1, dtype=torch.float32)
    view = base[1:].view(2, 8)                                # rows 4 bytes off the allocation's alignment
    assert view.data_ptr() % 16 == 4
    table = _call.as_table(view, "cpu")
    assert table.data_ptr() % 16 == 0 and table.dtype == torch.float32 and table.is_contiguous() and torch.equal(table, view)
    aligned = torch.ones(2, 8)
    assert _call.as_table(aligned, "cpu") is aligned          # nothing to do: no copy
    assert _call.as_table(np.ones((3, 4), np.float64), "cpu").dtype == torch.float32


def test_host_array():
    assert np.array_equal(_call.host_array(torch.tensor([3, 1])), [3, 1]) and isinstance(_call.host_array(torch.tensor([3, 1])), np.ndarray)
    assert _call.host_array([1, 2]).dtype.kind == "i" and _call.host_array([]).shape == (0,)
    a = np.arange(3)
    assert _call.host_array(a) is a


def test_workspace_has_the_size_the_library_reports():
    lib = _lib.load()
    Q, G, slab_rows, slabs = 70, 300, 64, 5                   # the size rule of tests/test_gpu_opensearch.py
    nbytes = _call.workspace_size(lib.fn_mate_search_workspace, "mate_search_workspace", Q, G, slab_rows)
    assert nbytes == slabs * Q * 20 + Q * 8
    ws = _call.workspace(torch.device("cpu"), lib.fn_mate_search_workspace, "mate_search_workspace", Q, G, slab_rows)
    assert ws.dtype == torch.int64 and ws.dim() == 1 and ws.numel() * 8 >= slabs * Q * 20 + Q * 8 and ws.numel() == -(-nbytes // 8)
    with pytest.raises(ValueError, match="mate_search_workspace") as err:
        _call.workspace(torch.device("cpu"), lib.fn_mate_search_workspace, "mate_search_workspace", 0, G, slab_rows)
    assert str(err.value) == lib.fn_last_error().decode()     # the library's own message


def test_range_words_decode_and_check():
    empty = torch.tensor([0x7f7fffff, 0x80800000 - 2 ** 32], dtype=torch.int32)        # what a kernel starts its range from
    lo, hi = (_call._decode_ord(v) for v in empty.tolist())
    assert lo == float(np.finfo(np.float32).max) and hi == -lo and lo > hi
    _call.check_unit_range(empty, 1.e-5)

    def key(x):                                               # the order-preserving int32 the kernels keep a float as
        bits = int(np.array([x], np.float32).view(np.int32)[0])
        return bits if bits >= 0 else bits ^ 0x7FFFFFFF

    for x in (0.0, 1.0, -1.0, 0.25, -1.0000119):
        assert _call._decode_ord(key(x)) == float(np.float32(x))
    _call.check_unit_range(torch.tensor([key(-1.0), key(1.0)], dtype=torch.int32), 1.e-5)
    with pytest.raises(ValueError, match="embeddings must be normalized to 1, range -1.0 1.5"):
        _call.check_unit_range(torch.tensor([key(-1.0), key(1.5)], dtype=torch.int32), 1.e-5)
    with pytest.raises(ValueError, match="embeddings must be normalized to 1"):
        _call.check_unit_range(torch.tensor([key(-1.25), key(1.0)], dtype=torch.int32), 1.e-5)
    from facenet_amd import statistics
    assert statistics._decode_ord is _call._decode_ord and statistics.check_unit_range is _call.check_unit_range


TEXTS = (("nlist", 1, 6, " (the gallery's rows)", r"nlist must be an integer in \[1, 6\] \(the gallery's rows\), got {}"),
         ("nprobe", 1, None, "", "nprobe must be an integer of at least 1, got {}"),
         ("iters", 0, None, "", "iters must be a non-negative integer, got {}"),
         ("min_samples", 1, None, "", "min_samples must be an integer of at least 1, got {}"),
         ("rank", 1, None, "", "rank must be an integer of at least 1, got {}"),
         ("k", 1, None, "", "k must be an integer of at least 1, got {}"))


@pytest.mark.parametrize("name, lo, hi, note, text", TEXTS, ids=[t[0] for t in TEXTS])
def test_check_int_keeps_every_text(name, lo, hi, note, text):
    for bad in (True, 2.5, lo - 1, None) + (() if hi is None else (hi + 1,)):
        with pytest.raises(ValueError, match="^" + text.format(repr(bad)) + "$"):
            _call.check_int(name, bad, lo, hi, note=note)
    got = _call.check_int(name, np.int64(3), lo, hi, note=note)
    assert got == 3 and type(got) is int
    assert _call.check_int(name, lo, lo, hi, note=note) == lo and (hi is None or _call.check_int(name, hi, lo, hi, note=note) == hi)
