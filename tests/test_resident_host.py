"""The decoded-pixel pack on disk (facenet_amd/resident.py), host side: the round trip against PIL's decode,
the file layout, when a pack is reused and when it is rebuilt, and what is refused.  No GPU needed."""
import os

import numpy as np
import pytest

from facenet_amd import resident
from facenet_amd.config import Config

SIZES = [(182, 182), (25, 40), (17, 5), (1, 1), (33, 35)]


def _write_db(root, classes, per_class, seed=0):
    from PIL import Image
    rng = np.random.default_rng(seed)
    truth = {}
    root.mkdir(exist_ok=True)
    for c in range(classes):
        d = root / f"id_{c:03d}"
        d.mkdir()
        for i in range(per_class):
            h, w = SIZES[(c * per_class + i) % len(SIZES)]
            arr = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
            f = d / f"img_{i:03d}.png"
            Image.fromarray(arr).save(f)
            truth[str(f)] = arr
    return truth


def _database(root, **keys):
    from facenet_amd import dataset
    return dataset.Database(Config({"path": str(root), **keys}))


def test_round_trip_layout_and_order(tmp_path):
    from PIL import Image
    truth = _write_db(tmp_path / "data", 3, 4)
    db = _database(tmp_path / "data")
    pack = resident.build_pack(db, tmp_path / "pack", workers=3)
    m = db.nrof_images
    assert pack.nrof_images == m == 12 and pack.version == resident.VERSION
    assert pack.files == [os.path.relpath(f, db.path) for f in db.files]
    assert np.array_equal(pack.labels, db.labels) and pack.labels.dtype == np.int64
    assert pack.classes == [c.name for c in db.classes]
    assert pack.hw.dtype == np.int32 and pack.hw.shape == (m, 2) and pack.offsets.dtype == np.int64 and pack.offsets.shape == (m + 1,)
    assert np.all(np.diff(pack.offsets) > 0) and np.all(pack.offsets % 16 == 0) and pack.offsets[0] == 0
    assert pack.offsets[m] == os.path.getsize(tmp_path / "pack" / resident.PIXELS) == pack.nbytes
    assert isinstance(pack.pixels, np.memmap)
    for i, f in enumerate(db.files):
        with Image.open(f) as im:
            want = np.asarray(im.convert("RGB"))
        assert np.array_equal(pack.image(i), want) and np.array_equal(want, truth[f]), f
        assert tuple(pack.hw[i]) == want.shape[:2]
        assert pack.offsets[i + 1] - pack.offsets[i] >= want.size
    st = [os.stat(f) for f in db.files]
    assert np.array_equal(pack.st_size, [s.st_size for s in st]) and np.array_equal(pack.st_mtime_ns, [s.st_mtime_ns for s in st])
    assert not [p for p in tmp_path.iterdir() if ".tmp." in p.name]            # the temporary directory was renamed, not left
    again = resident.Pack(tmp_path / "pack")
    assert again.matches(db) and np.array_equal(again.image(5), pack.image(5))


def test_one_image_set(tmp_path):
    truth = _write_db(tmp_path / "data", 1, 1)
    db = _database(tmp_path / "data")
    pack, hit = resident.ensure_pack(db, tmp_path / "pack")
    assert not hit and pack.nrof_images == 1 and pack.offsets.tolist() == [0, (182 * 182 * 3 + 15) // 16 * 16]
    assert np.array_equal(pack.image(0), truth[db.files[0]])


def test_decode_is_windowed(tmp_path):
    """The decode runs in windows sized from the largest image seen, not over the whole set at once."""
    _write_db(tmp_path / "data", 4, 10)
    db = _database(tmp_path / "data")
    files = db.files
    got = list(resident._decoded(files, workers=2, chunk_bytes=3 * 182 * 182 * 3))
    assert len(got) == len(files) and all(np.array_equal(a, resident._decode(f)) for a, f in zip(got, files))


def test_valid_pack_is_reused_and_a_changed_set_rebuilds_it(tmp_path, monkeypatch):
    from PIL import Image
    _write_db(tmp_path / "data", 3, 4)
    db = _database(tmp_path / "data")
    assert resident.ensure_pack(db, tmp_path / "pack")[1] is False
    stock = resident._decode
    calls = []

    def refusing(path):
        raise AssertionError(f"a valid pack must not decode {path}")

    monkeypatch.setattr(resident, "_decode", refusing)
    pack, hit = resident.ensure_pack(_database(tmp_path / "data"), tmp_path / "pack")
    assert hit and pack.nrof_images == 12

    def counting(path):
        calls.append(path)
        return stock(path)

    monkeypatch.setattr(resident, "_decode", counting)
    # one file's content and mtime change
    f = db.files[5]
    new = np.random.default_rng(9).integers(0, 256, (21, 30, 3), dtype=np.uint8)
    Image.fromarray(new).save(f)
    st = os.stat(f)
    os.utime(f, ns=(st.st_atime_ns, st.st_mtime_ns + 1_000_000_000))
    pack, hit = resident.ensure_pack(_database(tmp_path / "data"), tmp_path / "pack")
    assert not hit and len(calls) == 12 and np.array_equal(pack.image(5), new) and tuple(pack.hw[5]) == (21, 30)
    # a file is added
    calls.clear()
    Image.fromarray(new).save(tmp_path / "data" / "id_001" / "zz_added.png")
    db2 = _database(tmp_path / "data")
    pack, hit = resident.ensure_pack(db2, tmp_path / "pack")
    assert not hit and len(calls) == 13 and pack.nrof_images == 13 and pack.matches(db2) and not pack.matches(db)
    # max_nrof_images names a subset of every class
    calls.clear()
    np.random.seed(0)
    db3 = _database(tmp_path / "data", max_nrof_images=2)
    pack, hit = resident.ensure_pack(db3, tmp_path / "pack")
    assert not hit and len(calls) == 6 and pack.nrof_images == 6 and pack.files == [os.path.relpath(f, db3.path) for f in db3.files]
    calls.clear()
    assert resident.ensure_pack(db3, tmp_path / "pack")[1] is True and not calls


def test_truncated_pixels_wrong_version_and_leftover_temporary_directory(tmp_path):
    truth = _write_db(tmp_path / "data", 2, 3)
    db = _database(tmp_path / "data")
    # a leftover temporary directory of an interrupted build is not a pack: it is neither read nor in the way
    left = tmp_path / f"pack.tmp.{os.getpid()}"
    left.mkdir()
    (left / resident.PIXELS).write_bytes(b"\x00" * 100)
    with pytest.raises(FileNotFoundError):
        resident.Pack(tmp_path / "pack")
    pack, hit = resident.ensure_pack(db, tmp_path / "pack")
    assert not hit and pack.matches(db) and np.array_equal(pack.image(0), truth[db.files[0]])
    other = tmp_path / "pack.tmp.1"                     # another process's: left alone, ignored
    other.mkdir()
    assert resident.ensure_pack(db, tmp_path / "pack")[1] is True and other.exists()
    # a wrong version raises on opening and counts as invalid for the data set
    index = tmp_path / "pack" / resident.INDEX
    with np.load(index) as z:
        tables = {k: z[k] for k in z.files}
    del pack
    tables["version"] = np.int64(resident.VERSION + 1)
    with open(index, "wb") as f:
        np.savez(f, **tables)
    with pytest.raises(ValueError, match="version"):
        resident.Pack(tmp_path / "pack")
    pack, hit = resident.ensure_pack(db, tmp_path / "pack")
    assert not hit and pack.version == resident.VERSION
    # pixels shorter than the index says: refused, also by ensure_pack (the files have not changed, the pack is damaged)
    need = pack.nbytes
    del pack
    with open(tmp_path / "pack" / resident.PIXELS, "r+b") as f:
        f.truncate(need - 1)
    with pytest.raises(ValueError, match=str(need)):
        resident.Pack(tmp_path / "pack")
    with pytest.raises(ValueError, match=str(need)):
        resident.ensure_pack(db, tmp_path / "pack")


def _rank(rank, world, port, data, pack, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        decoded = []
        stock = resident._decode
        resident._decode = lambda f: (decoded.append(f), stock(f))[1]
        db = _database(data)
        first = resident.ensure_pack_collective(db, pack, rank)
        mine, hit = resident.ensure_pack(db, pack)              # what from_database does on every rank after the barrier
        q.put((rank, first, hit, len(decoded), mine.nrof_images))
    finally:
        dist.destroy_process_group()


def test_rank_zero_builds_and_every_rank_finds_the_pack_valid(tmp_path):
    """Two gloo ranks: only rank 0 decodes, the other waits at the barrier and then loads rank 0's pack."""
    import socket
    import torch.multiprocessing as mp
    _write_db(tmp_path / "data", 2, 3)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_rank, args=(r, 2, port, str(tmp_path / "data"), str(tmp_path / "pack"), q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=120) for _ in range(2))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert res == [(0, False, True, 6, 6), (1, None, True, 0, 6)]
    assert resident.ensure_pack_collective(_database(tmp_path / "data"), tmp_path / "pack", 0) is None      # no group: nothing to do
