"""Host half of the streaming loader (stream.py): header scan, the slot ring and its reader threads over ordinary
memory.  No GPU.  Every comparison is on bytes."""
import math
import threading
import time

import numpy as np
import pytest

import scene_net_amd as sna
from scene_net_amd import stream as st

N_FILES, BATCH = 32, 4


def _tile(rng, n, cols=4, dtype=np.float64):
    a = rng.standard_normal((n, cols))
    a[:, 0] += 5.44e5
    a[:, 1] += 4.634e6
    a[:, -1] = rng.integers(0, 20, n)
    return a.astype(dtype)


@pytest.fixture(scope="module")
def ragged(tmp_path_factory):
    """32 ragged (N,4) f64 tiles, N in 300..3000."""
    root = tmp_path_factory.mktemp("ragged")
    (root / "fit").mkdir()
    rng = np.random.default_rng(7)
    for k, n in enumerate(rng.integers(300, 3001, N_FILES)):
        np.save(root / "fit" / f"sample_{k:03d}.npy", _tile(rng, int(n)))
    return sna.TS40KTiles(str(root), "fit")


def _expected(ds, idx):
    """pack_csr(load_host(idx)), re-interleaved: rows [total,4] and offsets."""
    pts, lab, offsets, _ = sna.pack_csr(*ds.load_host(idx))
    return np.concatenate([pts, lab[:, None]], axis=1), offsets


def _slot_bytes(slot):
    return slot.rows[:slot.total].tobytes(), slot.offsets[:slot.n_tiles + 1].tobytes(), tuple(slot.files)


def _wait_threads(start, timeout):
    deadline = time.monotonic() + timeout
    while threading.active_count() > start and time.monotonic() < deadline:
        time.sleep(0.005)
    return threading.active_count()


# ---- scan -------------------------------------------------------------------------------------------------------------
def test_scan_tiles_flags_reasons_and_capacity(tmp_path):
    d = tmp_path / "fit"
    d.mkdir()
    rng = np.random.default_rng(0)
    np.save(d / "a_good0.npy", _tile(rng, 700))
    np.save(d / "a_good1.npy", _tile(rng, 1200))
    np.save(d / "b_f32.npy", _tile(rng, 900, dtype=np.float32))
    np.save(d / "c_five.npy", _tile(rng, 500, cols=5))
    np.save(d / "d_fortran.npy", np.asfortranarray(_tile(rng, 400)))
    np.save(d / "e_trunc.npy", _tile(rng, 5000))
    blob = (d / "e_trunc.npy").read_bytes()
    (d / "e_trunc.npy").write_bytes(blob[:len(blob) // 2])
    np.save(d / "f_empty.npy", np.zeros((0, 4)))
    np.save(d / "g_xyz.npy", rng.standard_normal((9000, 3)))
    (d / "x.npy").write_text("this is no npy file")
    (d / "notes.txt").write_text("ignored by the listing")
    ds = sna.TS40KTiles(str(tmp_path), "fit")
    infos = sna.scan_tiles(ds)
    by = {str(f): i for f, i in zip(ds.npy_files, infos)}
    assert set(by) == {"a_good0.npy", "a_good1.npy", "b_f32.npy", "c_five.npy", "d_fortran.npy", "e_trunc.npy",
                       "f_empty.npy", "g_xyz.npy", "x.npy"}
    for name, n, cols, dtype, fortran in (("a_good0.npy", 700, 4, "<f8", False), ("a_good1.npy", 1200, 4, "<f8", False),
                                          ("b_f32.npy", 900, 4, "<f4", False), ("c_five.npy", 500, 5, "<f8", False),
                                          ("d_fortran.npy", 400, 4, "<f8", True)):
        i = by[name]
        assert i.ok and i.reason == "" and (i.n_rows, i.cols, i.fortran) == (n, cols, fortran), name
        assert i.dtype == np.dtype(dtype)
        assert i.payload_offset > 0 and i.payload_offset % 16 == 0
    assert not by["e_trunc.npy"].ok and "file size" in by["e_trunc.npy"].reason and by["e_trunc.npy"].n_rows == 5000
    assert not by["f_empty.npy"].ok and by["f_empty.npy"].reason == "no rows"
    assert not by["g_xyz.npy"].ok and "3 columns" in by["g_xyz.npy"].reason
    assert not by["x.npy"].ok and by["x.npy"].reason.startswith("header")
    # capacity: the `batch_size` largest among the OK files (the truncated 5000 and the (N,3) 9000 do not count)
    assert st.capacity_points(infos, 2) == 1200 + 900
    assert st.capacity_points(infos, 3) == 1200 + 900 + 700
    assert st.capacity_points(infos, 50) == 700 + 1200 + 900 + 500 + 400
    ring = sna.TileRing(ds, 2, slots=2, readers=1)
    assert ring.capacity_points == 2100 and all(s.rows.shape == (2100, 4) for s in ring.slots)
    # the odd layouts are read to the same rows as the parent's loader gives
    order = [int(np.where(ds.npy_files == n)[0][0]) for n in ("b_f32.npy", "c_five.npy", "d_fortran.npy", "a_good0.npy")]
    ring = sna.TileRing(ds, 2, slots=2, readers=2, indices=order)
    got = [_slot_bytes(s) for s in ring.epoch(0)]
    assert len(got) == 2
    for k, (rows, offsets, files) in enumerate(got):
        exp_rows, exp_off = _expected(ds, order[2 * k:2 * k + 2])
        assert files == tuple(order[2 * k:2 * k + 2])
        assert rows == exp_rows.tobytes() and offsets == exp_off.tobytes()


# ---- ring -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def expected_in_order(ragged):
    exp = []
    for k in range(0, N_FILES, BATCH):
        rows, off = _expected(ragged, range(k, k + BATCH))
        exp.append((rows.tobytes(), off.tobytes(), tuple(range(k, k + BATCH))))
    return exp


@pytest.mark.parametrize("slots", [2, 3])
@pytest.mark.parametrize("readers", [1, 4])
def test_ring_content_equals_parent_loader(ragged, expected_in_order, slots, readers):
    start = threading.active_count()
    ring = sna.TileRing(ragged, BATCH, slots=slots, readers=readers, timeout_s=10)
    ptrs = [s.rows.ctypes.data for s in ring.slots]
    got = [_slot_bytes(s) for s in ring.epoch(0)]
    assert got == expected_in_order
    assert [_slot_bytes(s) for s in ring.epoch(1)] == expected_in_order   # not shuffled: every epoch alike
    assert [s.rows.ctypes.data for s in ring.slots] == ptrs                # the ring is never reallocated
    assert ring.skipped == []
    assert _wait_threads(start, 10) == start


def test_ring_limits(ragged):
    for kw in (dict(slots=2, readers=9), dict(slots=2, readers=0), dict(slots=1, readers=1)):
        with pytest.raises(ValueError):
            sna.TileRing(ragged, BATCH, **kw)


def test_shuffle_is_seeded_and_differs_between_epochs(ragged):
    def run(seed, epoch, readers):
        ring = sna.TileRing(ragged, BATCH, slots=3, readers=readers, shuffle=True, seed=seed, timeout_s=10)
        return [_slot_bytes(s) for s in ring.epoch(epoch)]
    a0, a0_again, a1, b0 = run(3, 0, 4), run(3, 0, 1), run(3, 1, 4), run(4, 0, 4)
    assert a0 == a0_again
    order0 = [i for _, _, files in a0 for i in files]
    assert order0 == [int(i) for i in np.random.default_rng(3).permutation(N_FILES)]
    assert sorted(order0) == list(range(N_FILES))
    assert [f for _, _, f in a1] != [f for _, _, f in a0] and [f for _, _, f in b0] != [f for _, _, f in a0]
    assert [i for _, _, files in a1 for i in files] == [int(i) for i in np.random.default_rng(4).permutation(N_FILES)]
    for rows, off, files in a1[:2]:
        exp_rows, exp_off = _expected(ragged, files)
        assert rows == exp_rows.tobytes() and off == exp_off.tobytes()


def test_indices_and_drop_last(ragged):
    idx = [5, 5, 31, 0, 17, 2, 9]
    ring = sna.TileRing(ragged, 3, slots=2, readers=4, indices=idx, timeout_s=10)
    got = [_slot_bytes(s) for s in ring.epoch(0)]
    assert [f for _, _, f in got] == [(5, 5, 31), (0, 17, 2), (9,)]
    rows, off = _expected(ragged, [9])
    assert got[2][0] == rows.tobytes() and got[2][1] == off.tobytes()
    ring = sna.TileRing(ragged, 3, slots=2, readers=4, indices=idx, drop_last=True, timeout_s=10)
    assert [tuple(s.files) for s in ring.epoch(0)] == [(5, 5, 31), (0, 17, 2)]


def test_slow_consumer_and_slow_readers_give_the_same_bytes(ragged, expected_in_order, monkeypatch):
    ring = sna.TileRing(ragged, BATCH, slots=2, readers=4, timeout_s=10)
    got = []
    for s in ring.epoch(0):          # consumer slower than the readers: they wait for FREE slots
        time.sleep(0.02)
        got.append(_slot_bytes(s))
    assert got == expected_in_order
    real = st._read_tile

    def slow(path, info, out):
        time.sleep(0.02)
        real(path, info, out)
    monkeypatch.setattr(st, "_read_tile", slow)
    ring = sna.TileRing(ragged, BATCH, slots=3, readers=4, timeout_s=10)
    assert [_slot_bytes(s) for s in ring.epoch(0)] == expected_in_order   # the consumer waits for FILLED slots


# ---- bad samples ------------------------------------------------------------------------------------------------------
@pytest.fixture()
def with_bad_files(tmp_path):
    d = tmp_path / "fit"
    d.mkdir()
    rng = np.random.default_rng(11)
    for k in range(10):
        np.save(d / f"sample_{k:03d}.npy", _tile(rng, int(rng.integers(300, 900))))
    blob = (d / "sample_003.npy").read_bytes()
    (d / "sample_003.npy").write_bytes(blob[:1000])            # truncated
    np.save(d / "sample_006.npy", rng.standard_normal((50, 3)))  # (N,3)
    return sna.TS40KTiles(str(tmp_path), "fit")


def _draw(seed, key, candidates):
    rng = np.random.default_rng(np.random.SeedSequence(seed, spawn_key=key))
    return candidates[int(rng.integers(len(candidates)))]


def test_bad_files_are_replaced_deterministically(with_bad_files):
    ds = with_bad_files
    runs = []
    for readers in (1, 4, 4):
        ring = sna.TileRing(ds, 4, slots=2, readers=readers, seed=5, timeout_s=10)
        got = [_slot_bytes(s) for s in ring.epoch(0)]
        runs.append((got, list(ring.skipped)))
    assert runs[0] == runs[1] == runs[2]
    got, skipped = runs[0]
    assert len(got) == math.ceil(10 / 4)
    assert [(i, f) for i, f, _ in skipped] == [(3, "sample_003.npy"), (6, "sample_006.npy")]
    assert "file size" in skipped[0][2] and "3 columns" in skipped[1][2]
    # a child stream of default_rng(5) per (epoch, batch, scan-time); drawn among the ok files the batch does not hold
    r3 = _draw(5, (0, 0, 0), [4, 5, 7, 8, 9])
    r6 = _draw(5, (0, 1, 0), [0, 1, 2, 8, 9])
    assert [f for _, _, f in got] == [(0, 1, 2, r3), (4, 5, r6, 7), (8, 9)]
    # the draw does not depend on what earlier epochs drew: epoch 0 again after epoch 1 gives the same files
    ring = sna.TileRing(ds, 4, slots=2, readers=4, seed=5, timeout_s=10)
    e1 = [tuple(s.files) for s in ring.epoch(1)]
    assert e1 == [(0, 1, 2, _draw(5, (1, 0, 0), [4, 5, 7, 8, 9])), (4, 5, _draw(5, (1, 1, 0), [0, 1, 2, 8, 9]), 7), (8, 9)]
    assert [tuple(s.files) for s in ring.epoch(0)] == [f for _, _, f in got]
    for rows, off, files in got:
        exp_rows, exp_off = _expected(ds, files)
        assert rows == exp_rows.tobytes() and off == exp_off.tobytes()


def test_late_read_failure_rebuilds_the_slot(with_bad_files):
    ds = with_bad_files
    ring = sna.TileRing(ds, 4, slots=2, readers=4, seed=5, indices=[0, 1, 2, 4, 5, 7, 8, 9], timeout_s=10)
    path = ring._path(5)                       # ok at the scan, truncated before the epoch reads it
    blob = open(path, "rb").read()
    open(path, "wb").write(blob[:len(blob) - 64])
    got = [_slot_bytes(s) for s in ring.epoch(0)]
    assert len(got) == 2 and [(i, f) for i, f, _ in ring.skipped] == [(5, "sample_005.npy")]
    assert ring.skipped[0][2].startswith("read:")
    rep = _draw(5, (0, 1, 1), [0, 1, 2, 4])          # (epoch 0, batch 1, late): ok files the batch does not hold
    assert got[0][2] == (0, 1, 2, 4) and got[1][2] == (rep, 7, 8, 9)
    for rows, off, files in got:
        exp_rows, exp_off = _expected(ds, files)
        assert rows == exp_rows.tobytes() and off == exp_off.tobytes()
    # from the next epoch on the file is not ok: replaced at plan time, never read (and rebuilt) again
    reads = []
    real = st._read_tile
    try:
        st._read_tile = lambda path, info, out: (reads.append(path), real(path, info, out))[1]
        files = [tuple(s.files) for s in ring.epoch(1)]
    finally:
        st._read_tile = real
    assert not ring.infos[5].ok and ring.infos[5].reason.startswith("read:")
    assert [(i, f) for i, f, _ in ring.skipped] == [(5, "sample_005.npy")] and not any(p.endswith("005.npy") for p in reads)
    assert files == [(0, 1, 2, 4), (_draw(5, (1, 1, 0), [0, 1, 2, 4]), 7, 8, 9)]


def test_two_slots_rebuilding_do_not_depend_on_timing(with_bad_files):
    ds = with_bad_files
    idx = [0, 1, 2, 4, 5, 7, 8, 9]
    originals = {}
    try:
        for i in (1, 7):                          # one late failure in each of the two batches
            path = sna.TileRing(ds, 4, indices=idx)._path(i)
            originals[path] = open(path, "rb").read()
        runs = []
        for readers in (1, 4, 4):
            ring = sna.TileRing(ds, 4, slots=2, readers=readers, seed=9, indices=idx, timeout_s=10)   # scanned while whole
            for path, blob in originals.items():
                open(path, "wb").write(blob[:len(blob) - 32])
            runs.append(([_slot_bytes(s) for s in ring.epoch(0)], ring.skipped))
            for path, blob in originals.items():
                open(path, "wb").write(blob)
        assert runs[0] == runs[1] == runs[2]
        got, skipped = runs[0]

        def rebuilt(batch_no, files, pos):            # the slot's own stream; a draw may land on the other bad file
            rng = np.random.default_rng(np.random.SeedSequence(9, spawn_key=(0, batch_no, 1)))
            files, gone = list(files), []
            while files[pos] in (1, 7):
                gone.append(files[pos])
                cands = [p for p in idx if p not in gone and p not in files[:pos] + files[pos + 1:]]
                files[pos] = cands[int(rng.integers(len(cands)))]
            return tuple(files), gone
        b0, gone0 = rebuilt(0, [0, 1, 2, 4], 1)
        b1, gone1 = rebuilt(1, [5, 7, 8, 9], 1)
        assert [f for _, _, f in got] == [b0, b1]
        assert sorted(i for i, _, _ in skipped) == sorted(gone0 + gone1) and {1, 7} <= {i for i, _, _ in skipped}
        for rows, off, files in got:
            exp_rows, exp_off = _expected(ds, files)
            assert rows == exp_rows.tobytes() and off == exp_off.tobytes()
    finally:
        for path, blob in originals.items():
            open(path, "wb").write(blob)


# ---- capacity ---------------------------------------------------------------------------------------------------------
@pytest.fixture()
def four_sizes(tmp_path):
    d = tmp_path / "fit"
    d.mkdir()
    rng = np.random.default_rng(3)
    for k, n in enumerate((100, 200, 300, 1000)):
        np.save(d / f"s{k}.npy", _tile(rng, n))
    return sna.TS40KTiles(str(tmp_path), "fit")


def test_repeated_indices_of_the_largest_file_fit_their_slot(four_sizes):
    ds = four_sizes
    idx = [3, 3, 0, 1]
    assert st.capacity_points(sna.scan_tiles(ds), 2) == 1300              # distinct files
    assert st.capacity_points(sna.scan_tiles(ds), 2, idx) == 2000         # the largest file is named twice
    ring = sna.TileRing(ds, 2, slots=2, readers=2, indices=idx, timeout_s=10)
    assert ring.capacity_points == 2000
    got = [_slot_bytes(s) for s in ring.epoch(0)]
    assert [f for _, _, f in got] == [(3, 3), (0, 1)]
    for rows, off, files in got:
        exp_rows, exp_off = _expected(ds, files)
        assert len(rows) == exp_rows.nbytes and rows == exp_rows.tobytes() and off == exp_off.tobytes()
    ring = sna.TileRing(ds, 2, slots=2, readers=2, indices=idx, shuffle=True, seed=1, timeout_s=10)
    for epoch in range(3):                                                  # wherever the two copies land
        for s in ring.epoch(epoch):
            exp_rows, exp_off = _expected(ds, s.files)
            assert s.total <= ring.capacity_points and _slot_bytes(s)[0] == exp_rows.tobytes()


def test_a_batch_that_does_not_fit_raises_instead_of_clipping(four_sizes):
    ds = four_sizes
    # too small a ring handed in: refused at construction
    with pytest.raises(ValueError):
        sna.TileRing(ds, 2, slots=2, indices=[3, 3, 0, 1], rows=[np.empty((1300, 4)) for _ in range(2)],
                     offsets=[np.zeros(3, dtype=np.int64) for _ in range(2)])
    # a replacement that has to repeat a file: only s3 is left, and two copies of it are more than a slot
    np.save(ds.dataset_path + "/s2.npy", np.zeros((5, 3)))
    ring = sna.TileRing(ds, 2, slots=2, indices=[3, 2], timeout_s=10)
    assert ring.capacity_points == 1000
    with pytest.raises(ValueError, match="holds 2000 rows, a slot 1000"):
        ring.start(0)
    ring.close()
    # the check the readers make when they open a slot, should a plan ever get past the first one
    ring = sna.TileRing(ds, 2, slots=2, indices=[0, 1], timeout_s=5)
    ring.plan_epoch = lambda epoch=0: [[3, 3]]
    ring.start(0)
    with pytest.raises(ValueError, match="holds 2000 rows"):
        ring.next()


def test_no_ok_file_raises(tmp_path):
    d = tmp_path / "fit"
    d.mkdir()
    np.save(d / "a.npy", np.zeros((10, 3)))
    (d / "b.npy").write_text("junk")
    with pytest.raises(RuntimeError, match="no readable tile"):
        sna.TileRing(sna.TS40KTiles(str(tmp_path), "fit"), 2)


# ---- failure handling -------------------------------------------------------------------------------------------------
def test_reader_exception_surfaces_in_the_consumer(ragged, monkeypatch):
    start = threading.active_count()
    real = st._read_tile

    def boom(path, info, out):
        if path.endswith("sample_009.npy"):
            raise KeyError("boom in a reader")
        real(path, info, out)
    monkeypatch.setattr(st, "_read_tile", boom)
    ring = sna.TileRing(ragged, BATCH, slots=2, readers=4, timeout_s=5)
    seen = 0
    with pytest.raises(KeyError, match="boom in a reader"):
        for _ in ring.epoch(0):
            seen += 1
    assert seen <= 2                                  # the file sits in the third batch
    assert _wait_threads(start, 5) == start


def test_waits_are_bounded(ragged):
    start = threading.active_count()
    ring = sna.TileRing(ragged, BATCH, slots=2, readers=4, timeout_s=0.5)
    t0 = time.monotonic()
    ring.start(0)
    held = [ring.next(), ring.next()]                 # never released: no slot becomes FREE again
    assert all(s.state == st.IN_FLIGHT for s in held)
    # The readers have been waiting for a FREE slot since they claimed the last tile of batch 1, before the second next()
    # returned.  The consumer's own wait starts 0.1 s later here, so only the READER's bound can fire first; its error is
    # what the consumer raises.
    time.sleep(0.1)
    with pytest.raises(TimeoutError, match="reader waited 0.5 s for slot 0 to become FREE"):
        ring.next()
    waited = time.monotonic() - t0                    # from the start of the epoch: the reader's wait lies inside it
    print(f"bounded wait: the reader's TimeoutError reached the consumer {waited:.3f} s after start at timeout_s = 0.5")
    assert 0.5 <= waited < 2.0
    assert _wait_threads(start, 5) == start


def test_threads_are_gone_after_exhaustion_break_and_exception(ragged):
    start = threading.active_count()
    ring = sna.TileRing(ragged, BATCH, slots=3, readers=4, timeout_s=5)
    assert sum(1 for _ in ring.epoch(0)) == N_FILES // BATCH
    assert _wait_threads(start, 5) == start
    ring.start(1)
    slot = ring.next()
    assert threading.active_count() > start
    ring.release(slot)
    ring.close()                                      # a `break` out of an epoch, then close()
    assert _wait_threads(start, 5) == start
    with pytest.raises(ZeroDivisionError):
        for _ in ring.epoch(2):
            raise ZeroDivisionError
    assert _wait_threads(start, 5) == start
    assert sum(1 for _ in ring.epoch(3)) == N_FILES // BATCH   # and the ring still works


def test_first_error_survives_a_reader_stuck_in_a_read(ragged, monkeypatch):
    """close() cannot join a reader that sits in a read; the consumer still gets the error that ended the epoch."""
    start = threading.active_count()
    unblock = threading.Event()
    real = st._read_tile

    def read(path, info, out):
        if path.endswith("sample_001.npy"):
            unblock.wait(10)
        elif path.endswith("sample_002.npy"):
            raise KeyError("boom while another reader is stuck")
        real(path, info, out)
    monkeypatch.setattr(st, "_read_tile", read)
    ring = sna.TileRing(ragged, BATCH, slots=2, readers=4, timeout_s=0.3)
    ring.start(0)
    try:
        with pytest.raises(KeyError, match="boom while another reader is stuck"):
            ring.next()
    finally:
        unblock.set()
    ring.close()
    assert _wait_threads(start, 5) == start
