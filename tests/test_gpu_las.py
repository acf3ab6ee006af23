"""LAS decode on the device (K13: sn_las_decode, scene_net_amd.las) against the numpy oracle of las_cases -- np.frombuffer
with the record dtype, `X * scale + offset`, the class rule, np.bincount.  Every comparison is bit for bit: fp64 as int64
views, counts as they are.  Every raw call decodes records that lie at a chosen residue mod 16 inside a larger buffer of
junk bytes, into sentinel-filled outputs with guard words on both sides."""
import io
import os
import pickle

import numpy as np
import pytest
import torch

import scene_net_amd as sna
from scene_net_amd import _hip

import las_cases as lc

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A5A5A5A5A
GUARD = 64
GRID_CAP = 2048      # csrc/las.hip kMaxBlocks: more chunks than this and a workgroup walks several
STAGED_MAX = 80      # csrc/las.hip kMaxStagedStride: longer records take the kernel that reads global memory directly


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _place(dev, raw, residue):
    """`raw` (uint8 array) on the device at an address that is `residue` mod 16, junk bytes in front of and behind it"""
    raw = np.ascontiguousarray(raw, dtype=np.uint8).reshape(-1)
    junk = np.random.default_rng(raw.size).integers(0, 256, raw.size + 160, dtype=np.uint8)
    big = torch.from_numpy(junk).to(dev)
    start = 64 + (residue - (big.data_ptr() + 64)) % 16
    big[start:start + raw.size] = torch.from_numpy(raw).to(dev)
    view = big[start:start + raw.size]
    assert view.data_ptr() % 16 == residue and view.is_contiguous()
    return big, view


def _guarded(words, dev, shift=0):
    """(whole int64 buffer, the `words` words inside it): GUARD sentinel words on both sides, the inside sentinel too;
    shift = 1 puts the inside on an address that is 8 but not 16 bytes aligned"""
    buf = torch.full((words + 2 * GUARD + shift,), SENTINEL, dtype=torch.int64, device=dev)
    assert buf.data_ptr() % 16 == 0
    return buf, buf[GUARD + shift:GUARD + shift + words]


def _check_guards(name, buf, inside, shift):
    b = buf.cpu().numpy()
    lo = GUARD + shift
    assert np.all(b[:lo] == SENTINEL) and np.all(b[lo + inside.numel():] == SENTINEL), f"{name}: guard words were written"


def _decode(dev, rows, fmt, residue=0, shift=0, scale=lc.SCALE, offset=lc.OFFSET, want_classes=True, want_hist=True,
            hist0=None, n=None):
    """sn_las_decode of rows [n, S] uint8 -> (pts bits [n,3] i64, classes bits [n] i64 | None, hist [256] i64 | None)"""
    rows = np.ascontiguousarray(rows, dtype=np.uint8)
    n = rows.shape[0] if n is None else n
    S = rows.shape[1]
    big, view = _place(dev, rows, residue)
    before = big.clone()
    p_buf, pts = _guarded(3 * n, dev, shift)
    c_buf, cls = _guarded(n, dev, shift)
    h_buf, hist = _guarded(256, dev, shift)
    hist.copy_(torch.zeros(256, dtype=torch.int64) if hist0 is None else torch.from_numpy(np.asarray(hist0, dtype=np.int64)))
    _hip.las_decode(view, n, fmt, S, scale, offset, pts.view(torch.float64), cls.view(torch.float64) if want_classes else None,
                    hist if want_hist else None)
    torch.cuda.synchronize()
    for name, buf, inside in (("pts", p_buf, pts), ("classes", c_buf, cls), ("hist", h_buf, hist)):
        _check_guards(name, buf, inside, shift)
    assert torch.equal(big, before), "the input bytes were written"
    if not want_classes:
        assert np.all(cls.cpu().numpy() == SENTINEL), "classes is not written when it is null"
    return (pts.cpu().numpy().reshape(n, 3), cls.cpu().numpy() if want_classes else None,
            hist.cpu().numpy() if want_hist else None)


def _assert_oracle(got, rows, fmt, scale=lc.SCALE, offset=lc.OFFSET, hist0=None, what="", n=None):
    n = rows.shape[0] if n is None else n
    pts, cls, hist = lc.decode_oracle(rows, n, fmt, rows.shape[1], scale, offset)
    assert np.array_equal(got[0], bits(pts)), f"{what}: pts"
    if got[1] is not None:
        assert np.array_equal(got[1], bits(cls)), f"{what}: classes"
    if got[2] is not None:
        assert np.array_equal(got[2], hist + (0 if hist0 is None else np.asarray(hist0))), f"{what}: hist"


# ---- 1. sizes on the seams of lanes, chunks and the grid ---------------------------------------------------------------
def _sizes():
    W = _hip.las_chunk_records()
    return [1, 2, 63, 64, 65, W - 1, W, W + 1, 2 * W + 1, GRID_CAP * W + W + 3]


@pytest.mark.parametrize("which", range(10))
def test_sizes_on_the_seams(hip_device, which):
    n = _sizes()[which]
    combos = [(0, 0), (3, 0), (6, 1), (10, 5)] if which < 9 else [(0, 0), (6, 1)]   # (format, extra bytes)
    for j, (fmt, extra) in enumerate(combos):
        rows = lc.random_records(n, fmt, extra, seed=which)
        residue, shift = (5 * which + 3 * j + 1) % 16, (which + j) % 2
        _assert_oracle(_decode(hip_device, rows, fmt, residue, shift), rows, fmt,
                       what=f"n={n} format {fmt}+{extra} residue {residue} shift {shift}")


# ---- 2. every format at its standard length and with 1, 3 and 5 bytes more ---------------------------------------------
@pytest.mark.parametrize("fmt", range(11))
def test_every_format_and_stride(hip_device, fmt):
    n = 2 * _hip.las_chunk_records() + 1
    parities = set()
    for extra in (0, 1, 3, 5):
        rows = lc.random_records(n, fmt, extra, seed=20 + fmt)
        assert rows.shape[1] == lc.STANDARD_LENGTH[fmt] + extra <= STAGED_MAX
        parities.add(rows.shape[1] % 2)
        residue = (7 * fmt + extra) % 16
        _assert_oracle(_decode(hip_device, rows, fmt, residue, (fmt + extra) % 2), rows, fmt, what=f"format {fmt}+{extra}")
    assert parities == {0, 1}


# ---- 3. every residue of the base address ------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt, extra", [(1, 0), (3, 0), (6, 0), (5, 0), (10, 1), (0, STAGED_MAX - 20), (0, STAGED_MAX - 19)])
def test_every_residue_of_the_base_address(hip_device, fmt, extra):
    n = _hip.las_chunk_records() + 1
    rows = lc.random_records(n, fmt, extra, seed=40 + fmt)
    want = lc.decode_oracle(rows, n, fmt, rows.shape[1], lc.SCALE, lc.OFFSET)
    for residue in range(16):
        got = _decode(hip_device, rows, fmt, residue, residue % 2)
        assert np.array_equal(got[0], bits(want[0])) and np.array_equal(got[1], bits(want[1])), f"residue {residue}"
        assert np.array_equal(got[2], want[2])


# ---- 4. records longer than the staged kernel takes: the direct kernel -------------------------------------------------
@pytest.mark.parametrize("S", [STAGED_MAX + 1, 97, 200, 1021, 65535])
def test_long_records(hip_device, S):
    W = _hip.las_chunk_records()
    for fmt, n, residue in ((2, W + 1, 13), (8, 2 * W + 1 if S < 2000 else 65, 6), (5, 1, 3)):
        if S < lc.STANDARD_LENGTH[fmt]:
            continue
        rows = lc.random_records(n, fmt, S - lc.STANDARD_LENGTH[fmt], seed=S)
        _assert_oracle(_decode(hip_device, rows, fmt, residue, n % 2), rows, fmt, what=f"record_length {S} format {fmt} n={n}")


def test_long_records_when_the_grid_wraps(hip_device):
    n = GRID_CAP * _hip.las_chunk_records() + 77
    rows = lc.random_records(n, 1, STAGED_MAX + 1 - 28, seed=5)
    _assert_oracle(_decode(hip_device, rows, 1, 9, 1), rows, 1, what="direct kernel, wrapped grid")


# ---- 5. coordinate values ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt, extra", [(0, 0), (3, 1), (6, 0), (7, 3), (1, 60)])
def test_coordinates_at_the_ends_of_int32(hip_device, fmt, extra):
    rows = lc.edge_records(fmt, extra, seed=fmt)
    for scale, offset in ((lc.SCALE, lc.OFFSET), ((1.0, 1e-9, 1e290), (0.0, -0.0, 1e290)), ((-0.01, 3.0, 1e-300), (1e15, 0.1, 5e-324))):
        got = _decode(hip_device, rows, fmt, 11, 1, scale, offset)
        _assert_oracle(got, rows, fmt, scale, offset, what=f"format {fmt}+{extra} scale {scale}")
    pts, _, _ = lc.decode_oracle(rows, 125, fmt, rows.shape[1], (1.0, 1.0, 1.0), (0.0, 0.0, 0.0))
    assert sorted(set(pts[:, 0].tolist())) == [float(v) for v in lc.INT32_EDGES]


# ---- 6. class bytes ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", range(11))
def test_every_value_of_the_class_byte(hip_device, fmt):
    for extra in (0, 3):
        rows = lc.class_records(fmt, extra, seed=fmt)
        got = _decode(hip_device, rows, fmt, (3 * fmt + 2) % 16, extra % 2)
        _assert_oracle(got, rows, fmt, what=f"format {fmt}+{extra}")
        want = (np.arange(256) & 31) if fmt <= 5 else np.arange(256)
        assert np.array_equal(got[1], bits(want.astype(np.float64)))
        assert np.array_equal(got[2], np.bincount(want, minlength=256))
        # the other candidate byte is no part of the answer: flip it everywhere
        other = rows.copy()
        other[:, 16 if fmt <= 5 else 15] ^= 0xFF
        again = _decode(hip_device, other, fmt, 1, 0)
        assert np.array_equal(again[1], got[1]) and np.array_equal(again[2], got[2])


# ---- 7. two roundings, never one ---------------------------------------------------------------------------------------
def test_the_product_is_rounded_before_the_sum(hip_device):
    X = lc.contraction_xs()
    (s0, o0), (s1, o1) = lc.CONTRACTION
    scale, offset = (s0, s1, s0), (o0, o1, -o0)
    for fmt, residue in ((1, 7), (6, 2)):
        rows = lc.set_xyz(lc.random_records(X.size, fmt, 0, seed=9), X, X[::-1], X)
        got = _decode(hip_device, rows, fmt, residue, 1, scale, offset)
        _assert_oracle(got, rows, fmt, scale, offset, what="contraction set")
        fused = [lc.fused_result(X, s0, o0), lc.fused_result(X[::-1], s1, o1)]
        for a in (0, 1):
            differs = int((got[0][:, a] != bits(fused[a])).sum())
            print(f"axis {a}: {differs} of {X.size} values differ from the singly rounded result")
            assert differs >= 100, "the set cannot tell a contracted multiply-add from two roundings"


# ---- 8. optional outputs, accumulation ---------------------------------------------------------------------------------
def test_optional_outputs(hip_device):
    n = 3 * _hip.las_chunk_records() + 5
    for fmt in (2, 9):
        rows = lc.random_records(n, fmt, 1, seed=fmt)
        for want_classes, want_hist in ((False, True), (True, False), (False, False)):
            got = _decode(hip_device, rows, fmt, 15, 1, want_classes=want_classes, want_hist=want_hist)
            assert (got[1] is None) == (not want_classes) and (got[2] is None) == (not want_hist)
            _assert_oracle(got, rows, fmt, what=f"classes {want_classes} hist {want_hist}")


def test_hist_is_accumulated_over_calls(hip_device):
    W = _hip.las_chunk_records()
    a, b = lc.random_records(2 * W + 9, 1, 0, seed=1), lc.random_records(W - 3, 1, 0, seed=2)
    start = np.arange(256, dtype=np.int64) * 1000 + 2**40
    first = _decode(hip_device, a, 1, 3, 0, hist0=start)
    _assert_oracle(first, a, 1, hist0=start, what="first call")
    second = _decode(hip_device, b, 1, 12, 1, hist0=first[2])
    _assert_oracle(second, b, 1, hist0=first[2], what="second call")
    both = np.concatenate([a, b])
    assert np.array_equal(second[2] - start, lc.decode_oracle(both, both.shape[0], 1, 28, lc.SCALE, lc.OFFSET)[2])


def test_fewer_records_than_the_buffers_hold(hip_device):
    rows = lc.random_records(700, 3, 0, seed=4)
    got = _decode(hip_device, rows, 3, 5, 1, n=300)      # (the guards sit right behind point 299)
    _assert_oracle(got, rows, 3, n=300, what="n below the buffer's rows")


# ---- 9. a captured launch replayed on a refilled buffer ----------------------------------------------------------------
def test_captured_replay_on_a_refilled_buffer(hip_device):
    n, fmt = 2 * _hip.las_chunk_records() + 31, 3
    cases = [lc.random_records(n, fmt, 0, seed=s) for s in (61, 62)]
    big, view = _place(hip_device, cases[0], 9)
    pts = torch.empty((n, 3), dtype=torch.float64, device=hip_device)
    cls = torch.empty((n,), dtype=torch.float64, device=hip_device)
    hist = torch.zeros(256, dtype=torch.int64, device=hip_device)
    _hip.las_decode(view, n, fmt, 34, lc.SCALE, lc.OFFSET, pts, cls, hist)      # (eager first: the kernel is loaded)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        hist.zero_()
        _hip.las_decode(view, n, fmt, 34, lc.SCALE, lc.OFFSET, pts, cls, hist)
    for rows in (cases[1], cases[0], cases[1]):
        view.copy_(torch.from_numpy(rows.reshape(-1)))
        pts.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        got = (pts.cpu().numpy().view(np.int64), cls.cpu().numpy().view(np.int64), hist.cpu().numpy())
        _assert_oracle(got, rows, fmt, what="replay")


# ---- 10. a buffer beyond 2^31 bytes ------------------------------------------------------------------------------------
def test_a_buffer_beyond_two_to_the_31_bytes(hip_device):
    fmt, S = 10, 72
    n = 2**31 // S + 1000
    assert n * S > 2**31
    big = torch.empty(n * S + 64, dtype=torch.uint8, device=hip_device)
    gen = torch.Generator(device=hip_device).manual_seed(7)
    big.random_(0, 256, generator=gen)                                 # every byte random
    start = 16 + (5 - big.data_ptr()) % 16
    view = big[start:start + n * S]
    assert view.data_ptr() % 16 == 5
    records = view.view(n, S)
    p_buf, pts = _guarded(3 * n, hip_device, 1)
    c_buf, cls = _guarded(n, hip_device, 1)
    hist = torch.zeros(256, dtype=torch.int64, device=hip_device)
    _hip.las_decode(view, n, fmt, S, lc.SCALE, lc.OFFSET, pts.view(torch.float64), cls.view(torch.float64), hist)
    torch.cuda.synchronize()
    assert bool((p_buf[:GUARD + 1] == SENTINEL).all()) and bool((p_buf[GUARD + 1 + 3 * n:] == SENTINEL).all())
    assert bool((c_buf[:GUARD + 1] == SENTINEL).all()) and bool((c_buf[GUARD + 1 + n:] == SENTINEL).all())
    assert torch.equal(hist, torch.bincount(records[:, 16].to(torch.int64), minlength=256))
    pts, cls = pts.view(n, 3), cls
    for name, sel in (("head", slice(0, 1000)), ("tail", slice(n - 1000, n)), ("sample", slice(0, n, 9973))):
        rows = records[sel].cpu().numpy()
        want = lc.decode_oracle(rows, rows.shape[0], fmt, S, lc.SCALE, lc.OFFSET)
        assert np.array_equal(pts[sel].cpu().numpy(), bits(want[0])), name
        assert np.array_equal(cls[sel].cpu().numpy(), bits(want[1])), name
    # the first record that starts beyond byte 2^31 of the buffer
    i = (2**31 - start) // S + 1
    rows = records[i:i + 3].cpu().numpy()
    assert np.array_equal(pts[i:i + 3].cpu().numpy(), bits(lc.decode_oracle(rows, 3, fmt, S, lc.SCALE, lc.OFFSET)[0]))


# ---- 11. LasReader -----------------------------------------------------------------------------------------------------
def _scan_equals(scan, rows, fmt, scale=lc.SCALE, offset=lc.OFFSET, what=""):
    want = lc.decode_oracle(rows, rows.shape[0], fmt, rows.shape[1], scale, offset)
    assert scan.xyz.shape == (rows.shape[0], 3) and scan.xyz.dtype == torch.float64 and scan.xyz.is_cuda
    assert np.array_equal(bits(scan.xyz.cpu().numpy()), bits(want[0])), f"{what}: xyz"
    assert np.array_equal(bits(scan.classes.cpu().numpy()), bits(want[1])), f"{what}: classes"
    assert scan.hist.dtype == torch.int64 and np.array_equal(scan.hist.cpu().numpy(), want[2]), f"{what}: hist"


def test_reader_gives_the_same_tensors_at_every_chunk_size(hip_device, tmp_path):
    fmt, n = 3, 1500
    rows = lc.random_records(n, fmt, 0, seed=70)
    path = str(tmp_path / "scan.las")
    off = lc.write_las(path, rows, fmt, minor=2, pad=6, trailing=b"behind the points")
    assert off % 2 == 1
    for chunk_bytes in (34, 1000, None):
        reader = sna.LasReader(hip_device) if chunk_bytes is None else sna.LasReader(hip_device, chunk_bytes=chunk_bytes)
        assert len(reader.plan(sna.read_las_header(path))) == {34: 1500, 1000: 52, None: 1}[chunk_bytes]
        scan = reader.read(path)
        torch.cuda.synchronize()
        _scan_equals(scan, rows, fmt, what=f"chunk_bytes {chunk_bytes}")
        assert scan.header.data_offset == off and sna.las_to_numpy(scan)[0] is scan.xyz
    plain = sna.read_las(path, hip_device, chunk_bytes=4096, want_classes=False, want_hist=False)
    assert plain.classes is None and plain.hist is None
    assert np.array_equal(bits(plain.xyz.cpu().numpy()), bits(lc.decode_oracle(rows, n, fmt, 34, lc.SCALE, lc.OFFSET)[0]))


def test_one_reader_two_files_the_second_shorter(hip_device, tmp_path):
    reader = sna.LasReader(hip_device, chunk_bytes=3000)
    a, b = lc.random_records(2000, 6, 0, seed=80), lc.random_records(333, 1, 3, seed=81)
    pa, pb = str(tmp_path / "a.las"), str(tmp_path / "b.las")
    lc.write_las(pa, a, 6, minor=4, pad=3)
    lc.write_las(pb, b, 1, minor=2, scale=(0.5, 0.25, 2.0), offset=(1.0, -2.0, 3.0))
    sa = reader.read(pa)
    sb = reader.read(pb)        # (no synchronisation in between: the buffers' events order the reuse)
    sa2 = reader.read(pa)
    torch.cuda.synchronize()
    _scan_equals(sa, a, 6, what="first file")
    _scan_equals(sb, b, 1, (0.5, 0.25, 2.0), (1.0, -2.0, 3.0), what="second, shorter file")
    _scan_equals(sa2, a, 6, what="first file again")
    with pytest.raises(_hip.HipLibraryError):
        sna.LasReader("cpu")


# ---- 12. build_data_samples --------------------------------------------------------------------------------------------
def test_build_data_samples_writes_what_the_crops_of_the_oracle_arrays_give(hip_device, tmp_path):
    scale, offset = (0.01, 0.01, 0.01), (5.0e5, 4.6e6, 100.0)
    las_dir, save_dir = tmp_path / "las", tmp_path / "out"
    las_dir.mkdir()
    towers = lc.scan_records(20000, 1, [(100.0, 100.0, 400), (300.0, 250.0, 350)], seed=1)
    plain = lc.scan_records(5000, 6, [], seed=2)
    lc.write_las(str(las_dir / "towers.las"), towers, 1, minor=2, scale=scale, offset=offset, pad=1)
    lc.write_las(str(las_dir / "plain.las"), plain, 6, minor=4, scale=scale, offset=offset)
    (las_dir / "notes.txt").write_text("not a scan")
    pts, cls, hist = lc.decode_oracle(towers, towers.shape[0], 1, 28, scale, offset)
    assert hist[15] == 750 and lc.decode_oracle(plain, 5000, 6, 30, scale, offset)[2][15] == 0
    want = sna.crop_tower_samples(torch.from_numpy(pts).to(hip_device), torch.from_numpy(cls).to(hip_device))
    assert len(want) == 2 and all(w.shape[1] == 4 and w.shape[0] >= 300 for w in want)

    with torch.cuda.device(hip_device):
        sna.build_data_samples([str(las_dir)], str(save_dir), data_split=0)
    assert sorted(os.listdir(save_dir / "fit")) == ["sample_0.npy", "sample_1.npy"]
    for k, w in enumerate(want):
        f = io.BytesIO()
        np.save(f, w.cpu().numpy())
        assert (save_dir / "fit" / f"sample_{k}.npy").read_bytes() == f.getvalue(), f"sample {k}"
        assert np.load(save_dir / "fit" / f"sample_{k}.npy").dtype == np.float64
    with open(save_dir / "read_files.pickle", "rb") as f:
        names = pickle.load(f)
    base = os.path.realpath(las_dir)
    assert sorted(names) == [base + "/plain.las", base + "/towers.las"]

    # a second run resumes: nothing is read again, and the two samples are split by the reference's slices
    stamp = {p: os.stat(save_dir / "fit" / p).st_mtime_ns for p in os.listdir(save_dir / "fit")}
    with torch.cuda.device(hip_device):
        sna.build_data_samples([str(las_dir)], str(save_dir), data_split={"fit": .5, "test": .5}, seed=3)
    assert len(os.listdir(save_dir / "fit")) == 1 and len(os.listdir(save_dir / "test")) == 1
    for folder in ("fit", "test"):
        for p in os.listdir(save_dir / folder):
            assert os.stat(save_dir / folder / p).st_mtime_ns == stamp[p]
    with open(save_dir / "read_files.pickle", "rb") as f:
        assert sorted(pickle.load(f)) == sorted(names)
