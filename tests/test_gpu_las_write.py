"""LAS encode on the device (K15: sn_las_encode, scene_net_amd.las_write) against the numpy oracle of las_write_cases --
np.rint((x - offset) / scale), the class rule, the fields assigned to las_cases.record_dtype.  Every comparison is byte for
byte.  Every raw call writes into a 16-byte aligned slice of a larger buffer filled with 0xA5, guard bytes on both sides,
and reads inputs that start one element into their allocations: at their element type's alignment and no more."""
import os

import numpy as np
import pytest
import torch

import scene_net_amd as sna
from scene_net_amd import _hip

import las_cases as lc
import las_write_cases as wc

pytestmark = pytest.mark.gpu

FILL = 0xA5
GUARD = 64


def _shifted(a, dev):
    """the array on the device as t[1:] of an allocation one element (row) longer: 8-byte alignment for f64, 2-byte for u16"""
    if a is None:
        return None
    a = np.ascontiguousarray(a)
    junk = np.full((1,) + a.shape[1:], 7, dtype=a.dtype)
    t =torch.from_numpy(np.concatenate([junk, a])).to(dev)[1:]
    assert t.is_contiguous() and t.data_ptr() % (2 if a.dtype == np.uint16 else 8) == 0
    return t


def _tensors(inp, dev):
    return {k: _shifted(v, dev) for k, v in inp.items()}


def _stats(dev, box0=wc.EMPTY_BOX, hist0=None, bad0=(0, 0)):
    return (torch.tensor(box0, dtype=torch.int32, device=dev),
            torch.zeros(256, dtype=torch.int64, device=dev) if hist0 is None else torch.from_numpy(np.asarray(hist0)).to(dev),
            torch.tensor(bad0, dtype=torch.int64, device=dev))


def _encode(dev, inp, fmt, extra=0, scale=lc.SCALE, offset=lc.OFFSET, stats=None, want_stats=True):
    """sn_las_encode of the inputs -> (rows [n,S] uint8, box tuple, hist [256], bad tuple); checks the guards"""
    n = inp["xyz"].shape[0]
    S = lc.STANDARD_LENGTH[fmt] + extra
    t = _tensors(inp, dev)
    big = torch.full((GUARD + n * S + GUARD + 16,), FILL, dtype=torch.uint8, device=dev)
    assert big.data_ptr() % 16 == 0 and GUARD % 16 == 0
    records = big[GUARD:]
    box, hist, bad = stats if stats is not None else _stats(dev)
    if not want_stats:
        box = hist = bad = None
    _hip.las_encode(t["xyz"], n, fmt, S, scale, offset, records, t["classes"], t["intensity"], t["gps"], t["rgb"], box, hist, bad)
    torch.cuda.synchronize()
    got = big.cpu().numpy()
    assert np.all(got[:GUARD] == FILL), "bytes in front of the records were written"
    assert np.all(got[GUARD + n * S:] == FILL), "bytes behind the last record were written"
    rows = got[GUARD:GUARD + n * S].reshape(n, S)
    if not want_stats:
        return rows, None, None, None
    return rows, tuple(box.cpu().tolist()), hist.cpu().numpy(), tuple(bad.cpu().tolist())


def _assert_oracle(got, want, what=""):
    assert got[0].shape == want[0].shape, what
    if not np.array_equal(got[0], want[0]):
        i, j = np.argwhere(got[0] != want[0])[0]
        raise AssertionError(f"{what}: record {i} byte {j}: got {got[0][i].tolist()} want {want[0][i].tolist()}")
    if got[1] is not None:
        assert got[1] == want[1], f"{what}: box {got[1]} != {want[1]}"
        assert np.array_equal(got[2], want[2]), f"{what}: hist"
        assert got[3] == want[3], f"{what}: bad {got[3]} != {want[3]}"


def _sizes():
    C = _hip.las_encode_chunk_records()
    return [1, C - 1, C, C + 1, 2 * C + 3]


# ---- 1. parity: every served format, record lengths up to 80, sizes on the seams, with and without the optional arrays ----
@pytest.mark.parametrize("fmt", wc.SERVED)
def test_parity_with_the_oracle(hip_device, fmt):
    extras = [0, 1, 3, wc.MAX_RECORD_LENGTH - lc.STANDARD_LENGTH[fmt]]
    for which, n in enumerate(_sizes()):
        for extra in extras:
            for optional in (True, False):
                inp = wc.random_inputs(n, fmt, seed=10 * which + extra, optional=optional)
                want = wc.oracle_of(inp, fmt, extra)
                assert want[3] == (0, 0)
                _assert_oracle(_encode(hip_device, inp, fmt, extra), want, f"format {fmt}+{extra} n={n} optional {optional}")
    assert lc.STANDARD_LENGTH[fmt] + extras[-1] == 80


def test_statistics_are_optional(hip_device):
    inp = wc.random_inputs(700, 3, seed=2)
    got = _encode(hip_device, inp, 3, 1, want_stats=False)
    _assert_oracle(got, wc.oracle_of(inp, 3, 1), "no box, hist, bad")


def test_the_grid_wraps(hip_device):
    n = 2048 * _hip.las_encode_chunk_records() + 300        # csrc/las_write.hip kMaxBlocks: some workgroups walk two chunks
    inp = wc.random_inputs(n, 0, seed=5, optional=False)
    inp["classes"] = (np.arange(n) % 32).astype(np.float64)
    _assert_oracle(_encode(hip_device, inp, 0, 1), wc.oracle_of(inp, 0, 1), "wrapped grid")


# ---- 2. rounding and saturation ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [1, 6])
def test_rounding_and_saturation(hip_device, fmt):
    scale, offset = (0.001, 0.001, 0.001), (0.0, 0.0, 0.0)
    xyz = wc.rounding_xyz(0.001)
    assert wc.reciprocal_differs(xyz[:, 0], 0.001) > 0, "the set cannot tell a division from a reciprocal"
    inp = {"xyz": xyz, "classes": None, "intensity": None, "gps": None, "rgb": None}
    want = wc.oracle_of(inp, fmt, 0, scale, offset)
    assert want[3][0] > 10 and want[3][1] == 0 and want[1][0] == -2**31 and want[1][1] == 2**31 - 1
    # bad counts points: fewer than the coordinates that are out of range
    assert want[3][0] < sum(int(wc.quantise(xyz[:, a], 0.001, 0.0)[1].sum()) for a in range(3))
    _assert_oracle(_encode(hip_device, inp, fmt, 0, scale, offset), want, f"format {fmt}")
    # another scale and a non-zero offset: the subtraction is rounded on its own
    inp2 = {**inp, "xyz": wc.tie_inputs(0.0001, 5000)[:, None] * np.ones(3) + np.array(lc.OFFSET)}
    sc2 = (0.0001, 0.0001, 0.0001)
    _assert_oracle(_encode(hip_device, inp2, fmt, 0, sc2, lc.OFFSET), wc.oracle_of(inp2, fmt, 0, sc2, lc.OFFSET), "offset set")


# ---- 3. classes --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [1, 3, 6, 8])
def test_classes_the_format_cannot_hold(hip_device, fmt):
    c = np.tile(np.array(wc.CLASS_VALUES), 30)[:333]
    inp = wc.random_inputs(c.shape[0], fmt, seed=4)
    inp["classes"] = c
    want = wc.oracle_of(inp, fmt, 0)
    top = 31 if fmt <= 5 else 255
    assert want[3][1] == int(sum(1 for v in c if not (v == v and v == np.floor(v) and 0 <= v <= top))) > 0
    assert want[2][0] > want[3][1] and want[2].sum() == c.shape[0]
    got = _encode(hip_device, inp, fmt, 0)
    _assert_oracle(got, want, f"format {fmt}")
    assert set(got[0][:, 15 if fmt <= 5 else 16].tolist()) == ({0, 15, 31} if fmt <= 5 else {0, 15, 31, 32, 80, 255})
    if fmt > 5:
        assert np.all(got[0][:, 15] == 0)


# ---- 4. nothing outside: every residue of n * S mod 16 -----------------------------------------------------------------
def _residue_cases():
    C = _hip.las_encode_chunk_records()
    return [(3, 1, C + j) for j in range(16)] + [(0, 1, j) for j in range(1, 17)] + [(6, 0, 2 * C + j) for j in range(8)]


def test_nothing_outside_at_every_residue_of_the_length(hip_device):
    cases = _residue_cases()
    residues = {}
    for fmt, extra, n in cases:
        residues.setdefault((n * (lc.STANDARD_LENGTH[fmt] + extra)) % 16, []).append((fmt, extra, n))
    assert sorted(residues) == list(range(16)), "the case list misses a residue of n * S mod 16"
    for fmt, extra, n in cases:
        inp = wc.random_inputs(n, fmt, seed=n)
        _assert_oracle(_encode(hip_device, inp, fmt, extra), wc.oracle_of(inp, fmt, extra), f"format {fmt}+{extra} n={n}")


def test_misaligned_records_are_refused(hip_device):
    buf = torch.zeros(256, dtype=torch.uint8, device=hip_device)
    xyz = torch.zeros((1, 3), dtype=torch.float64, device=hip_device)
    with pytest.raises(_hip.HipLibraryError, match="16-byte"):
        _hip.las_encode(xyz, 1, 0, 20, lc.SCALE, lc.OFFSET, buf[8:])
    with pytest.raises(_hip.HipLibraryError):
        _hip.las_encode(xyz.cpu(), 1, 0, 20, lc.SCALE, lc.OFFSET, buf)
    torch.cuda.synchronize()
    assert not bool(buf.any())


# ---- 5. accumulation ---------------------------------------------------------------------------------------------------
def test_two_calls_over_the_halves_equal_one_call_over_the_whole(hip_device):
    n, fmt = 2 * _hip.las_encode_chunk_records() + 77, 3
    inp = wc.random_inputs(n, fmt, seed=8)
    inp["xyz"][5, 0], inp["xyz"][n - 3, 2], inp["classes"][7], inp["classes"][n - 1] = np.nan, np.inf, 99.0, -1.0
    whole = _encode(hip_device, inp, fmt, 0)
    want = wc.oracle_of(inp, fmt, 0)
    assert want[3] == (2, 2)
    _assert_oracle(whole, want, "whole")
    h = n // 2 + 1
    halves = [{k: (None if v is None else v[s]) for k, v in inp.items()} for s in (slice(0, h), slice(h, n))]
    stats = _stats(hip_device)
    a = _encode(hip_device, halves[0], fmt, 0, stats=stats)
    _assert_oracle(a, wc.oracle_of(halves[0], fmt, 0), "first half")
    b = _encode(hip_device, halves[1], fmt, 0, stats=stats)
    assert b[1] == whole[1] and np.array_equal(b[2], whole[2]) and b[3] == whole[3]
    assert np.array_equal(np.concatenate([a[0], b[0]]), whole[0])


# ---- 6. a captured launch replayed on overwritten inputs ---------------------------------------------------------------
def test_captured_replay_on_overwritten_inputs(hip_device):
    n, fmt, S = 2 * _hip.las_encode_chunk_records() + 31, 3, 34
    cases = [wc.random_inputs(n, fmt, seed=s) for s in (61, 62)]
    t = {k: torch.from_numpy(v).to(hip_device) for k, v in cases[0].items()}
    records = torch.empty(n * S, dtype=torch.uint8, device=hip_device)
    box, hist, bad = _stats(hip_device)
    fresh = _stats(hip_device)

    def launch():
        _hip.las_encode(t["xyz"], n, fmt, S, lc.SCALE, lc.OFFSET, records, t["classes"], t["intensity"], t["gps"], t["rgb"],
                        box, hist, bad)

    launch()                                                                    # (eager first: the kernel is loaded)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch()
    for inp in (cases[1], cases[0], cases[1]):
        for k, v in inp.items():
            t[k].copy_(torch.from_numpy(v))
        for dst, src in zip((box, hist, bad), fresh):
            dst.copy_(src)
        records.fill_(FILL)
        graph.replay()
        torch.cuda.synchronize()
        got = (records.cpu().numpy().reshape(n, S), tuple(box.cpu().tolist()), hist.cpu().numpy(), tuple(bad.cpu().tolist()))
        _assert_oracle(got, wc.oracle_of(inp, fmt, 0), "replay")


# ---- 7. LasWriter ------------------------------------------------------------------------------------------------------
def _payload(path, header):
    with open(path, "rb") as f:
        f.seek(header.data_offset)
        return np.frombuffer(f.read(), dtype=np.uint8).reshape(header.n_points, header.record_length)


def test_writer_file_equals_the_oracle_and_reads_back(hip_device, tmp_path):
    n, fmt = 1000, 3
    inp = wc.random_inputs(n, fmt, seed=90, scale=(0.001,) * 3, offset=(100.0, 200.0, -5.0))
    t = {k: torch.from_numpy(v).to(hip_device) for k, v in inp.items()}
    path = str(tmp_path / "out.las")
    writer = sna.LasWriter(hip_device, chunk_bytes=4096)
    S = 34 + 1
    assert len(writer.plan(n, S)) >= 5
    head = writer.write(path, t["xyz"], t["classes"], t["intensity"], t["gps"], t["rgb"], point_format=fmt,
                        scale=(0.001,) * 3, offset=(100.0, 200.0, -5.0), extra_bytes=1)
    want = wc.oracle_of(inp, fmt, 1, (0.001,) * 3, (100.0, 200.0, -5.0))
    assert isinstance(head, sna.LasWritten) and isinstance(head, sna.LasHeader)
    assert (head.n_points, head.point_format, head.record_length, head.version) == (n, fmt, S, (1, 2))
    assert head.scale == (0.001,) * 3 and head.offset == (100.0, 200.0, -5.0)
    assert head.data_offset == head.header_size == 227 and head.file_size == 227 + n * S
    assert head.box == want[1] and np.array_equal(np.array(head.hist), want[2]) and head.bad == (0, 0)
    assert head.bbox == sna.las_write.box_to_bbox(want[1], head.scale, head.offset)
    assert np.array_equal(_payload(path, head), want[0]), "the file's records differ from the oracle's"
    assert not os.path.exists(path + ".part")
    scan = sna.read_las(path, hip_device)
    pts, cls, hist = lc.decode_oracle(want[0], n, fmt, S, head.scale, head.offset)
    assert np.array_equal(scan.xyz.cpu().numpy().view(np.int64), pts.view(np.int64))
    assert np.array_equal(scan.classes.cpu().numpy(), cls) and np.array_equal(scan.hist.cpu().numpy(), hist)
    # the header's box is the box of what a reader sees
    assert head.bbox == (pts[:, 0].max(), pts[:, 0].min(), pts[:, 1].max(), pts[:, 1].min(), pts[:, 2].max(), pts[:, 2].min())
    # the same writer again, another file, defaults: format 1 with gps_time, scale 0.001, offset floor(min)
    near = np.random.default_rng(91).uniform(-500.0, 500.0, (300, 3)) + np.array([4.2e6, 5.0e5, 80.0])
    head2 = writer.write(str(tmp_path / "b.las"), torch.from_numpy(near).to(hip_device), t["classes"][:300],
                         gps_time=t["gps"][:300])
    lo = np.floor(near.min(axis=0))
    assert head2.point_format == 1 and head2.scale == (0.001,) * 3 and head2.offset == tuple(lo.tolist())
    sub = {"xyz": near, "classes": inp["classes"][:300], "intensity": None, "gps": inp["gps"][:300], "rgb": None}
    assert np.array_equal(_payload(head2.path, head2), wc.oracle_of(sub, 1, 0, head2.scale, head2.offset)[0])
    assert head2.bad == (0, 0)


def test_default_format_moves_to_the_modern_ones_for_classes_above_31(hip_device, tmp_path):
    xyz = torch.rand((50, 3), dtype=torch.float64, device=hip_device)
    cls = torch.arange(50, dtype=torch.float64, device=hip_device)
    rgb = torch.zeros((50, 3), dtype=torch.uint16, device=hip_device)
    assert sna.write_las(str(tmp_path / "a.las"), xyz[:32], cls[:32]).point_format == 0
    assert sna.write_las(str(tmp_path / "b.las"), xyz, cls).point_format == 6
    assert sna.write_las(str(tmp_path / "c.las"), xyz, cls, rgb=rgb).version == (1, 4)
    assert sna.write_las(str(tmp_path / "d.las"), xyz, cls % 32, rgb=rgb).point_format == 2
    got = sna.read_las(str(tmp_path / "b.las"), hip_device)
    assert torch.equal(got.classes, cls) and got.header.record_length == 30


def test_like_reproduces_the_integers_of_the_file_it_came_from(hip_device, tmp_path):
    for fmt, minor in ((1, 2), (6, 4)):
        n = 700
        rows = lc.random_records(n, fmt, 0, seed=33 + fmt)
        if fmt <= 5:
            rows[:, 15] &= 31                      # no flag bits: the writer writes none
        src, dst = str(tmp_path / f"src{fmt}.las"), str(tmp_path / f"dst{fmt}.las")
        lc.write_las(src, rows, fmt, minor=minor, pad=3)
        scan = sna.read_las(src, hip_device)
        head = sna.write_las(dst, scan.xyz, scan.classes, like=scan.header, chunk_bytes=5000)
        assert (head.point_format, head.scale, head.offset, head.record_length) == (fmt, lc.SCALE, lc.OFFSET, rows.shape[1])
        got = _payload(dst, head)
        assert np.array_equal(got[:, :12], rows[:, :12]), "X, Y, Z"
        col = 15 if fmt <= 5 else 16
        assert np.array_equal(got[:, col], rows[:, col]), "class bytes"
        assert head.bad == (0, 0)


def test_strict_refuses_a_nan_and_leaves_no_file(hip_device, tmp_path):
    xyz = torch.rand((600, 3), dtype=torch.float64, device=hip_device)
    xyz[411, 1] = float("nan")
    cls = torch.full((600,), 40.0, dtype=torch.float64, device=hip_device)
    path = str(tmp_path / "bad.las")
    with pytest.raises(ValueError, match="1 points.*600 classes"):
        sna.write_las(path, xyz, cls, point_format=1, chunk_bytes=4096)
    assert not os.path.exists(path) and not os.path.exists(path + ".part") and os.listdir(tmp_path) == []
    head = sna.write_las(path, xyz, cls, point_format=1, chunk_bytes=4096, strict=False)
    assert head.bad == (1, 600) and head.hist[0] == 600 and head.n_points == 600
    with pytest.raises(_hip.HipLibraryError):
        sna.write_las(path, xyz.cpu())


def test_an_empty_scan_gives_a_header_only_file(hip_device, tmp_path):
    path = str(tmp_path / "empty.las")
    head = sna.write_las(path, torch.empty((0, 3), dtype=torch.float64, device=hip_device))
    assert head.n_points == 0 and head.file_size == 227 == os.path.getsize(path) and head.bbox == (0.0,) * 6
    scan = sna.read_las(path, hip_device)
    assert scan.xyz.shape == (0, 3) and scan.classes.shape == (0,)


# ---- 8. reclassify_las -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt, minor", [(1, 2), (3, 3), (7, 4), (10, 4)])
def test_reclassify_keeps_every_other_byte(hip_device, tmp_path, fmt, minor):
    n = 2000
    rows = lc.random_records(n, fmt, 2, seed=fmt)
    src, dst = str(tmp_path / "src.las"), str(tmp_path / "dst.las")
    off = lc.write_las(src, rows, fmt, minor=minor, pad=5, trailing=bytes(range(91)))
    new = np.random.default_rng(fmt).integers(0, 32 if fmt <= 5 else 256, n)
    head = sna.reclassify_las(src, dst, torch.from_numpy(new.astype(np.float64)).to(hip_device), chunk_bytes=7000)
    a, b = np.fromfile(src, dtype=np.uint8), np.fromfile(dst, dtype=np.uint8)
    assert a.shape == b.shape and head.n_points == n and head.data_offset == off
    col = 15 if fmt <= 5 else 16
    same = np.ones(a.shape, dtype=bool)
    same[off + col:off + n * rows.shape[1]:rows.shape[1]] = False
    assert np.array_equal(a[same], b[same]), "a byte that is no class byte changed"
    got = b[off:off + n * rows.shape[1]].reshape(n, -1)[:, col]
    if fmt <= 5:
        assert np.array_equal(got & 31, new) and np.array_equal(got & 0xE0, rows[:, col] & 0xE0)
    else:
        assert np.array_equal(got, new)
    assert not os.path.exists(dst + ".part")


def test_reclassify_refusals(hip_device, tmp_path):
    rows = lc.random_records(100, 1, 0, seed=1)
    src, dst = str(tmp_path / "src.las"), str(tmp_path / "dst.las")
    lc.write_las(src, rows, 1)
    c = torch.zeros(100, dtype=torch.float64, device=hip_device)
    c[17] = 40.0
    with pytest.raises(ValueError, match="0..31"):
        sna.reclassify_las(src, dst, c)
    assert not os.path.exists(dst) and not os.path.exists(dst + ".part")
    with pytest.raises(ValueError, match="100 points"):
        sna.reclassify_las(src, dst, c[:99])
    with pytest.raises(ValueError, match="same file"):
        sna.reclassify_las(src, src, c * 0)
    with pytest.raises(_hip.HipLibraryError):
        sna.reclassify_las(src, dst, c.cpu())
    assert not os.path.exists(dst)
