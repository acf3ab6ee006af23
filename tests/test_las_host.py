"""LAS decode (K13), host side: the header parser against files written by las_cases.write_las, the numpy oracle against
hand-written records, the contraction sets, the chunk plan and the split arithmetic of build_data_samples.  No GPU."""
import math
import struct
from fractions import Fraction

import numpy as np
import pytest

import scene_net_amd as sna
from scene_net_amd import las as sl

import las_cases as lc


def _file(tmp_path, name="a.las", fmt=1, n=7, extra=0, **kw):
    rows = lc.random_records(n, fmt, extra, seed=3)
    path = str(tmp_path / name)
    off = lc.write_las(path, rows, fmt, **kw)
    return path, rows, off


# ---- header parser: valid files ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("minor", [0, 1, 2, 3, 4])
def test_header_of_every_version(tmp_path, minor):
    path, rows, off = _file(tmp_path, fmt=3, n=11, extra=3, minor=minor, pad=5)
    h = sna.read_las_header(path)
    assert h.version == (1, minor) and h.header_size == lc.HEADER_SIZE[minor] and h.data_offset == off == h.header_size + 5
    assert (h.point_format, h.record_length, h.n_points) == (3, 37, 11)
    assert h.scale == lc.SCALE and h.offset == lc.OFFSET
    assert h.bbox == (6.0, 5.0, 4.0, 3.0, 2.0, 1.0)          # as read: max x, min x, max y, min y, max z, min z
    assert h.file_size == off + 11 * 37 and h.payload_bytes == 11 * 37


def test_u64_count_when_the_legacy_count_is_zero(tmp_path):
    path, _, _ = _file(tmp_path, fmt=1, n=9, minor=4, legacy_count=0)
    assert sna.read_las_header(path).n_points == 9


def test_u64_count_for_format_6_and_above_whatever_the_legacy_count_says(tmp_path):
    path, _, _ = _file(tmp_path, fmt=7, n=9, minor=4, legacy_count=4)
    h = sna.read_las_header(path)
    assert (h.point_format, h.record_length, h.n_points) == (7, 36, 9)


def test_legacy_count_wins_for_a_legacy_format_in_1_4(tmp_path):
    rows = lc.random_records(9, 1, 0, seed=1)
    path = str(tmp_path / "b.las")
    lc.write_las(path, rows, 1, minor=4, legacy_count=5, n=9)
    assert sna.read_las_header(path).n_points == 5


def test_trailing_records_behind_the_points_are_legal(tmp_path):
    path, _, off = _file(tmp_path, fmt=6, n=4, minor=4, trailing=bytes(range(97)))
    h = sna.read_las_header(path)
    assert h.n_points == 4 and h.file_size == off + 4 * 30 + 97


def test_any_residue_of_the_data_offset(tmp_path):
    for pad in range(16):
        path, _, off = _file(tmp_path, name=f"p{pad}.las", fmt=0, n=2, pad=pad)
        assert sna.read_las_header(path).data_offset == 227 + pad == off


# ---- header parser: rejections -----------------------------------------------------------------------------------------
def test_truncated_payload(tmp_path):
    path, rows, off = _file(tmp_path, fmt=1, n=7)
    with open(path, "r+b") as f:
        f.truncate(off + 7 * 28 - 1)
    with pytest.raises(ValueError, match="truncated"):
        sna.read_las_header(path)


def test_truncated_payload_of_a_u64_count(tmp_path):
    rows = lc.random_records(3, 6, 0, seed=1)
    path = str(tmp_path / "c.las")
    lc.write_las(path, rows, 6, minor=4, n=2**40)
    with pytest.raises(ValueError, match="truncated"):
        sna.read_las_header(path)


@pytest.mark.parametrize("bits", [0x80, 0x40, 0xC0])
def test_compressed_bit(tmp_path, bits):
    path, _, _ = _file(tmp_path, fmt=1, format_byte=1 | bits)
    with pytest.raises(ValueError, match="LAZ"):
        sna.read_las_header(path)


def test_bad_signature(tmp_path):
    path, _, _ = _file(tmp_path, signature=b"LASX")
    with pytest.raises(ValueError, match="signature"):
        sna.read_las_header(path)
    short = tmp_path / "short.las"
    short.write_bytes(b"LASF" + bytes(100))
    with pytest.raises(ValueError, match="no LAS header"):
        sna.read_las_header(str(short))


def test_format_above_10(tmp_path):
    path, _, _ = _file(tmp_path, fmt=1, format_byte=11)
    with pytest.raises(ValueError, match="above 10"):
        sna.read_las_header(path)


@pytest.mark.parametrize("fmt", range(11))
def test_short_record_length(tmp_path, fmt):
    rows = lc.random_records(3, 0, lc.STANDARD_LENGTH[fmt] - 21, seed=1) if fmt else np.zeros((3, 19), dtype=np.uint8)
    assert rows.shape[1] == lc.STANDARD_LENGTH[fmt] - 1
    path = str(tmp_path / "s.las")
    lc.write_las(path, rows, fmt, minor=4)
    with pytest.raises(ValueError, match="record length"):
        sna.read_las_header(path)


@pytest.mark.parametrize("minor", [0, 1, 2, 3, 4])
def test_header_size_too_small_for_its_version(tmp_path, minor):
    path, _, _ = _file(tmp_path, minor=minor, header_size=lc.HEADER_SIZE[minor] - 1, data_offset=lc.HEADER_SIZE[minor])
    with pytest.raises(ValueError, match="header size"):
        sna.read_las_header(path)


def test_unknown_version_and_data_inside_the_header(tmp_path):
    path, _, _ = _file(tmp_path, name="v.las", major=2)
    with pytest.raises(ValueError, match="version"):
        sna.read_las_header(path)
    path, _, _ = _file(tmp_path, name="d.las", data_offset=226)
    with pytest.raises(ValueError, match="inside"):
        sna.read_las_header(path)


@pytest.mark.parametrize("which", range(6))
@pytest.mark.parametrize("bad", [math.inf, -math.inf, math.nan])
def test_scale_or_offset_not_finite(tmp_path, which, bad):
    scale, offset = list(lc.SCALE), list(lc.OFFSET)
    (scale if which < 3 else offset)[which % 3] = bad
    path, _, _ = _file(tmp_path, scale=scale, offset=offset)
    with pytest.raises(ValueError, match="not finite"):
        sna.read_las_header(path)


# ---- the oracle against hand-written records ---------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", range(11))
def test_oracle_equals_hand_written_values(fmt):
    X, Y, Z = 123456789, -2147483648, 7
    body = struct.pack("<iiiHB", X, Y, Z, 0xBEEF, 0x5A)                   # bytes 0..14
    if fmt <= 5:
        body += struct.pack("<BbBH", 0xE0 | 15, -3, 9, 77)               # byte 15: three flag bits over class 15
        want_class = 15.0
    else:
        body += struct.pack("<BBBhH", 0xFF, 200, 9, -300, 77)            # byte 15: flags; byte 16: class 200
        body += struct.pack("<d", 1.5)
        want_class = 200.0
    S = lc.STANDARD_LENGTH[fmt]
    body += bytes((37 * i + fmt) % 256 for i in range(S - len(body)))    # whatever else the format holds
    assert len(body) == S
    scale, offset = (0.001, 0.01, 0.5), (4.2e6, 500000.0, -1.25)
    pts, cls, hist = lc.decode_oracle(body, 1, fmt, S, scale, offset)
    want = [float(np.float64(np.float64(v) * np.float64(s)) + np.float64(o)) for v, s, o in zip((X, Y, Z), scale, offset)]
    assert pts.tolist() == [want]
    assert want[2] == 2.25 and want[1] == 500000.0 - 21474836.48         # (both exact or singly rounded by hand)
    assert cls.tolist() == [want_class]
    assert hist.sum() == 1 and hist[int(want_class)] == 1
    # extra bytes change nothing
    pts2, cls2, _ = lc.decode_oracle(body + b"\xff\xff\xff", 1, fmt, S + 3, scale, offset)
    assert np.array_equal(pts2, pts) and np.array_equal(cls2, cls)


def test_oracle_drops_the_flag_bits_of_the_legacy_formats_only():
    for fmt in range(11):
        _, cls, hist = lc.decode_oracle(lc.class_records(fmt), 256, fmt, lc.STANDARD_LENGTH[fmt], lc.SCALE, lc.OFFSET)
        want = (np.arange(256) & 31) if fmt <= 5 else np.arange(256)
        assert np.array_equal(cls, want.astype(np.float64))
        assert np.array_equal(hist, np.bincount(want, minlength=256))


# ---- the contraction set -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale, offset", lc.CONTRACTION)
def test_the_contraction_set_tells_one_rounding_from_two(scale, offset):
    X = lc.contraction_xs()
    assert X.min() < -2**30 and X.max() > 2**30
    differs = lc.contraction_differs(X, scale, offset)
    print(f"scale {scale} offset {offset}: {differs} of {X.size} values differ between one rounding and two")
    assert differs >= 100
    # the fused result really is the exact one, rounded once
    x = int(X[0])
    exact = Fraction(x) * Fraction(scale) + Fraction(offset)
    f = lc.fused_result(X[:1], scale, offset)[0]
    assert abs(Fraction(f) - exact) <= abs(Fraction(np.nextafter(f, math.inf)) - exact)
    assert abs(Fraction(f) - exact) <= abs(Fraction(np.nextafter(f, -math.inf)) - exact)


# ---- chunk planning ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, S, chunk", [(1, 28, 64 << 20), (1000, 34, 1000), (1000, 34, 34), (1000, 34, 1), (7, 65535, 65535),
                                         (10**7, 28, 64 << 20), (29, 28, 28 * 29), (30, 28, 28 * 29), (0, 28, 100)])
def test_chunks_are_whole_records_at_least_one_and_the_last_is_short(n, S, chunk):
    plan = sna.plan_chunks(n, S, chunk)
    per = max(1, chunk // S)
    assert [c for _, c in plan[:-1]] == [per] * max(0, len(plan) - 1)
    assert all(c >= 1 for _, c in plan)
    assert [f for f, _ in plan] == list(range(0, n, per))
    assert sum(c for _, c in plan) == n
    if plan:
        assert 1 <= plan[-1][1] <= per and plan[-1][1] == n - per * (len(plan) - 1)
    assert all(c * S <= max(chunk, S) for _, c in plan)


def test_chunk_plan_refuses_nonsense():
    for args in ((5, 0, 10), (5, 28, 0), (-1, 28, 10)):
        with pytest.raises(ValueError):
            sna.plan_chunks(*args)


# ---- the split of build_data_samples -----------------------------------------------------------------------------------
def _reference_slices(sample_size, data_split):
    """core/datasets/ts40k.py:130-144, restated: the slice of `samples` every folder but 'fit' receives"""
    got, split_sum = {}, 0
    for folder, split in data_split.items():
        if folder == "fit":
            split_sum += split
            continue
        got[folder] = (int(split_sum * sample_size), math.ceil((split_sum + split) * sample_size))
        split_sum += split
    return got


@pytest.mark.parametrize("split", [{"fit": .6, "test": .4}, {"fit": .7, "val": .1, "test": .2}, {"test": .25, "fit": .5},
                                   {"fit": 1.0}, {"fit": .6, "test": .3}])
def test_split_counts_equal_the_references_slices(split):
    for size in (0, 1, 2, 3, 7, 10, 11, 99, 100, 101, 1234):
        got = sna.split_slices(size, split)
        assert got == _reference_slices(size, split)
        assert all(0 <= a <= b <= size for a, b in got.values())
    assert sna.split_slices(10, {"fit": .6, "test": .4}) == {"test": (6, 10)}
    assert sna.split_slices(11, {"fit": .7, "val": .1, "test": .2}) == {"val": (7, 9), "test": (8, 11)}   # (they overlap: so does the reference)


def test_module_surface():
    for name in ("read_las_header", "LasReader", "read_las", "las_to_numpy", "build_data_samples", "LasScan", "LasHeader"):
        assert hasattr(sna, name) and name in sna.__all__
    assert sl.LAS_STANDARD_LENGTH == lc.STANDARD_LENGTH and sl.LAS_HEADER_SIZE == lc.HEADER_SIZE
    with pytest.raises(TypeError):
        sna.las_to_numpy(object())


def test_entry_argument_checks_need_no_gpu():
    import ctypes
    from scene_net_amd import _hip
    lib = _hip.load()
    buf = ctypes.create_string_buffer(256)
    p = ctypes.cast(buf, ctypes.c_void_p)
    ok3 = (ctypes.c_double * 3)(0.01, 0.01, 0.01)
    s3 = ctypes.cast(ok3, ctypes.c_void_p)

    def call(records=p, n=1, fmt=0, S=20, scale=s3, offset=s3, pts=p, classes=p, hist=p):
        return lib.sn_las_decode(records, n, fmt, S, scale, offset, pts, classes, hist, None)

    assert call(records=None) == -1 and b"records" in lib.sn_last_error()
    assert call(pts=None) == -1
    assert call(n=0) == -1 and call(n=-5) == -1
    assert call(fmt=-1) == -1 and call(fmt=11) == -1
    for fmt, std in enumerate(lc.STANDARD_LENGTH):
        assert call(fmt=fmt, S=std - 1) == -1 and b"record_length" in lib.sn_last_error()
    assert call(S=65536) == -1
    for bad in (math.inf, -math.inf, math.nan):
        for i in range(3):
            v = (ctypes.c_double * 3)(0.01, 0.01, 0.01)
            v[i] = bad
            assert call(scale=ctypes.cast(v, ctypes.c_void_p)) == -1 and b"finite" in lib.sn_last_error()
            assert call(offset=ctypes.cast(v, ctypes.c_void_p)) == -1
    odd = ctypes.c_void_p(p.value + 4)
    assert call(pts=odd) == -1 and b"aligned" in lib.sn_last_error()
    assert call(classes=odd) == -1
    assert call(hist=odd) == -1
    assert _hip.las_chunk_records() == lib.sn_las_chunk_records() >= 64
