"""LAS encode (K15), host side: the numpy oracle of las_write_cases against K13's decode oracle and against hand-written
records, the tie set that tells a division from a product with the reciprocal, las_header_bytes against read_las_header,
the argument checks of sn_las_encode and the byte patch of reclassify_las.  No GPU."""
import ctypes
import math
import struct

import numpy as np
import pytest

import scene_net_amd as sna
from scene_net_amd import las_write as lw

import las_cases as lc
import las_write_cases as wc


# ---- the oracle ------------------------------------------------------------------------------------------------------
def test_decode_encode_decode_returns_the_integers():
    n = 200_000
    rng = np.random.default_rng(15)
    X = np.concatenate([rng.integers(-2**31, 2**31, size=(n, 3), dtype=np.int64),
                        np.array(np.meshgrid(lc.INT32_EDGES, lc.INT32_EDGES, lc.INT32_EDGES)).reshape(3, -1).T])
    rows = lc.set_xyz(lc.random_records(X.shape[0], 1, 0, seed=1), X[:, 0], X[:, 1], X[:, 2])
    pts, cls, _ = lc.decode_oracle(rows, X.shape[0], 1, 28, lc.SCALE, lc.OFFSET)
    back, box, hist, bad = wc.encode_oracle(pts, cls, None, None, None, 1, 0, lc.SCALE, lc.OFFSET)
    rec = back.reshape(-1).view(lc.record_dtype(1))
    for a, name in enumerate("XYZ"):
        mismatches = int((rec[name] != X[:, a]).sum())
        print(f"{name}: {mismatches} of {X.shape[0]} integers differ after decode and encode")
        assert mismatches == 0
    assert bad == (0, 0) and box == (-2**31, 2**31 - 1) * 3
    again = lc.decode_oracle(back, X.shape[0], 1, 28, lc.SCALE, lc.OFFSET)
    assert np.array_equal(again[0].view(np.int64), pts.view(np.int64)) and np.array_equal(again[1], cls)
    assert np.array_equal(again[2], hist)


@pytest.mark.parametrize("scale", [0.001, 0.0001])
def test_the_tie_set_tells_a_division_from_a_reciprocal(scale):
    x = wc.tie_inputs(scale)
    differs = wc.reciprocal_differs(x, scale)
    print(f"scale {scale}: {differs} of {x.size} inputs quantise differently with a reciprocal")
    assert differs > 0
    assert wc.reciprocal_differs(wc.rounding_xyz(0.001)[:, 0], 0.001) > 0      # the set the GPU test uses


@pytest.mark.parametrize("fmt", wc.SERVED)
def test_oracle_equals_hand_written_bytes(fmt):
    scale, offset = (0.001, 0.01, 0.5), (4.2e6, 500000.0, -1.25)
    xyz = np.array([[4.2e6 + 123.4565, 500000.0 - 21474836.48, 2.25]])
    X = [int(np.rint((np.float64(v) - np.float64(o)) / np.float64(s))) for v, s, o in zip(xyz[0], scale, offset)]
    assert X[1] == -2147483648 and X[2] == 7 and X[0] in (123456, 123457)
    gps = np.array([1.5]) if fmt in wc.GPS_FORMATS else None
    rgb = np.array([[0x1122, 0x3344, 0x5566]], dtype=np.uint16) if fmt in wc.RGB_FORMATS else None
    rows, box, hist, bad = wc.encode_oracle(xyz, np.array([21.0]), np.array([0xBEEF], dtype=np.uint16), gps, rgb, fmt, 3,
                                            scale, offset)
    body = struct.pack("<iiiH", X[0], X[1], X[2], 0xBEEF)
    if fmt <= 5:
        body += struct.pack("<BBbBH", 0x09, 21, 0, 0, 0)
    else:
        body += struct.pack("<BBBBhH", 0x11, 0, 21, 0, 0, 0)
    if gps is not None:
        body += struct.pack("<d", 1.5)
    if rgb is not None:
        body += struct.pack("<HHH", 0x1122, 0x3344, 0x5566)
    if fmt == 8:
        body += struct.pack("<H", 0)
    assert len(body) == lc.STANDARD_LENGTH[fmt]
    assert rows.tobytes() == body + bytes(3)
    assert box == (X[0], X[0], X[1], X[1], X[2], X[2]) and bad == (0, 0) and hist[21] == 1 and hist.sum() == 1


def test_oracle_saturates_and_counts_points_not_coordinates():
    # scale 0.5, offset 1: every quotient below is exact
    q = np.array([[np.nan, 0.0, 0.0], [np.inf, -np.inf, np.nan], [0.5, -0.5, 1.5], [2.5, -2.5, 3.5],
                  [2147483647.0, -2147483648.0, 2147483646.5], [2147483647.5, 0.0, 0.0], [0.0, -2147483648.5, 0.0],
                  [-2147483647.5, 5.0, 6.0]])
    xyz = q * 0.5 + 1.0
    assert np.array_equal(((xyz - 1.0) / 0.5)[2:], q[2:])
    rows, box, hist, bad = wc.encode_oracle(xyz, None, None, None, None, 0, 0, (0.5,) * 3, (1.0,) * 3)
    rec = rows.reshape(-1).view(lc.record_dtype(0))
    assert rec["X"].tolist() == [0, 2**31 - 1, 0, 2, 2**31 - 1, 2**31 - 1, 0, -2**31]
    assert rec["Y"].tolist() == [0, -2**31, 0, -2, -2**31, 0, -2**31, 5]
    assert rec["Z"].tolist() == [0, 0, 2, 4, 2**31 - 2, 0, 0, 6]
    assert bad == (4, 0)                                  # points 0, 1, 5 and 6: one each, whatever the number of coordinates
    assert box == (-2**31, 2**31 - 1, -2**31, 5, 0, 2**31 - 2)
    assert np.all(rec["class_bits"] == 0) and np.all(rec["return_bits"] == 0x09) and hist[0] == 8 and hist.sum() == 8


def test_oracle_class_rule():
    c = np.array(wc.CLASS_VALUES)
    n = c.shape[0]
    for fmt, top in ((1, 31), (6, 255)):
        rows, _, hist, bad = wc.encode_oracle(np.zeros((n, 3)), c, None, None, None, fmt, 0, lc.SCALE, lc.OFFSET)
        got = rows[:, 15 if fmt <= 5 else 16]
        want = [int(v) if (v == v and math.isfinite(v) and v == math.floor(v) and 0 <= v <= top) else 0 for v in c]
        assert got.tolist() == want
        assert bad[1] == sum(1 for v in c if not (v == v and math.isfinite(v) and v == math.floor(v) and 0 <= v <= top))
        assert np.array_equal(hist, np.bincount(want, minlength=256))
        if fmt > 5:
            assert np.all(rows[:, 15] == 0)


# ---- the header ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt, version", [(f, v) for f in wc.SERVED for v in (None, (1, 2), (1, 4)) if not (f >= 6 and v == (1, 2))])
def test_header_round_trip(tmp_path, fmt, version):
    S, n = lc.STANDARD_LENGTH[fmt] + 2, 12345
    box = (-5, 1000, -2**31, 2**31 - 1, 7, 7)
    head = sna.las_header_bytes(fmt, S, n, lc.SCALE, lc.OFFSET, box, version=version, creation=(293, 2026))
    minor = 4 if (fmt >= 6 or version == (1, 4)) else 2
    assert len(head) == lc.HEADER_SIZE[minor] == (375 if minor == 4 else 227)
    path = tmp_path / "h.las"
    path.write_bytes(head + bytes(n * S))
    h = sna.read_las_header(str(path))
    assert h.version == (1, minor) and h.header_size == h.data_offset == len(head)
    assert (h.point_format, h.record_length, h.n_points) == (fmt, S, n)
    assert h.scale == lc.SCALE and h.offset == lc.OFFSET
    want = []
    for a in range(3):
        v = np.array(box[2 * a:2 * a + 2], dtype=np.int32) * np.float64(lc.SCALE[a]) + np.float64(lc.OFFSET[a])
        want += [float(v[1]), float(v[0])]
    assert h.bbox == tuple(want)
    # the fields read_las_header does not return
    assert head[:4] == b"LASF" and struct.unpack_from("<HH", head, 4) == (0, 0x10 if minor == 4 else 0)
    assert head[26:58].rstrip(b"\0") == lw.SYSTEM_IDENTIFIER and head[58:90].rstrip(b"\0").startswith(b"scene_net_amd")
    assert struct.unpack_from("<HH", head, 90) == (293, 2026)
    assert struct.unpack_from("<I", head, 100)[0] == 0                       # no variable length records
    legacy = struct.unpack_from("<I5I", head, 107)
    assert legacy == ((n, n, 0, 0, 0, 0) if fmt <= 5 else (0,) * 6)
    if minor == 4:
        assert struct.unpack_from("<QQI", head, 227) == (0, 0, 0)
        assert struct.unpack_from("<Q15Q", head, 247) == (n, n) + (0,) * 14
    assert sna.las_header_bytes(fmt, S, n, lc.SCALE, lc.OFFSET, box, version=version) == \
        sna.las_header_bytes(fmt, S, n, lc.SCALE, lc.OFFSET, box, version=version)
    assert struct.unpack_from("<HH", sna.las_header_bytes(fmt, S, n, lc.SCALE, lc.OFFSET, box, version=version), 90) == (0, 0)


def test_header_refusals_and_the_empty_box():
    ok = dict(scale=lc.SCALE, offset=lc.OFFSET, box_xyz=wc.EMPTY_BOX)
    for fmt in (4, 5, 9, 10, 11, -1):
        with pytest.raises(ValueError):
            sna.las_header_bytes(fmt, 80, 1, **ok)
    with pytest.raises(ValueError):
        sna.las_header_bytes(1, 27, 1, **ok)
    with pytest.raises(ValueError):
        sna.las_header_bytes(1, 28, 2**32, **ok)
    with pytest.raises(ValueError):
        sna.las_header_bytes(6, 30, 5, version=(1, 2), **ok)
    with pytest.raises(ValueError):
        sna.las_header_bytes(1, 28, 5, version=(1, 3), **ok)
    with pytest.raises(ValueError):
        sna.las_header_bytes(1, 28, 5, scale=(0.1, math.nan, 0.1), offset=lc.OFFSET, box_xyz=wc.EMPTY_BOX)
    big = sna.las_header_bytes(6, 30, 2**32 + 5, **ok)
    assert struct.unpack_from("<Q", big, 247)[0] == 2**32 + 5 and struct.unpack_from("<I", big, 107)[0] == 0
    assert struct.unpack_from("<6d", sna.las_header_bytes(0, 20, 0, **ok), 179) == (0.0,) * 6


def test_module_surface():
    for name in ("LasWriter", "LasWritten", "write_las", "reclassify_las", "las_header_bytes"):
        assert hasattr(sna, name) and name in sna.__all__
    assert lw.LAS_WRITE_FORMATS == wc.SERVED and lw.LAS_WRITE_MAX_RECORD_LENGTH == wc.MAX_RECORD_LENGTH
    with pytest.raises(sna.HipLibraryError):
        sna.LasWriter("cpu")


# ---- sn_las_encode's argument checks -----------------------------------------------------------------------------------
def test_entry_argument_checks_need_no_gpu():
    from scene_net_amd import _hip
    lib = _hip.load()
    buf = ctypes.create_string_buffer(512)
    base = ctypes.addressof(buf)
    p = ctypes.c_void_p(base + (-base) % 16)
    ok3 = (ctypes.c_double * 3)(0.01, 0.01, 0.01)
    s3 = ctypes.cast(ok3, ctypes.c_void_p)
    INVALID, UNSUPPORTED = -1, -2

    def call(pts=p, classes=p, intensity=None, gps=None, rgb=None, n=1, fmt=0, S=None, scale=s3, offset=s3, records=p,
             box=p, hist=p, bad=p):
        S = lc.STANDARD_LENGTH[fmt] if S is None and 0 <= fmt <= 10 else (20 if S is None else S)
        return lib.sn_las_encode(pts, classes, intensity, gps, rgb, n, fmt, S, scale, offset, records, box, hist, bad, None)

    def at(k):
        return ctypes.c_void_p(p.value + k)

    assert call(pts=None) == INVALID and b"pts" in lib.sn_last_error()
    assert call(records=None) == INVALID and b"records" in lib.sn_last_error()
    assert call(scale=None) == INVALID and call(offset=None) == INVALID
    assert call(n=0) == INVALID and call(n=-5) == INVALID
    assert call(fmt=-1) == INVALID and call(fmt=11) == INVALID
    for fmt, std in enumerate(lc.STANDARD_LENGTH):
        assert call(fmt=fmt, S=std - 1) == INVALID and b"record_length" in lib.sn_last_error()
    for bad in (math.inf, -math.inf, math.nan, 0.0, -0.0):
        for i in range(3):
            v = (ctypes.c_double * 3)(0.01, 0.01, 0.01)
            v[i] = bad
            assert call(scale=ctypes.cast(v, ctypes.c_void_p)) == INVALID and b"scale" in lib.sn_last_error()
            if bad != 0.0:
                assert call(offset=ctypes.cast(v, ctypes.c_void_p)) == INVALID and b"offset" in lib.sn_last_error()
    for fmt in (0, 2):
        assert call(fmt=fmt, gps=p) == INVALID and b"gps_time" in lib.sn_last_error()
    for fmt in (0, 1, 6):
        assert call(fmt=fmt, rgb=p) == INVALID and b"rgb" in lib.sn_last_error()
    for k in (1, 2, 4, 8):
        assert call(records=at(k)) == INVALID and b"16-byte" in lib.sn_last_error()
    for name in ("pts", "classes", "hist", "bad"):
        assert call(**{name: at(4)}) == INVALID and b"aligned" in lib.sn_last_error(), name
    assert call(fmt=1, gps=at(4)) == INVALID
    assert call(box=at(2)) == INVALID
    assert call(intensity=at(1)) == INVALID and call(fmt=2, rgb=at(1)) == INVALID
    for fmt in (4, 5, 9, 10):
        assert call(fmt=fmt) == UNSUPPORTED and b"waveform" in lib.sn_last_error()
    for fmt in wc.SERVED:
        assert call(fmt=fmt, S=81) == UNSUPPORTED and b"record_length" in lib.sn_last_error()
    assert call(n=2**36 + 1) == UNSUPPORTED
    assert _hip.las_encode_chunk_records() == lib.sn_las_encode_chunk_records() >= 64


# ---- reclassify_las's byte patch -------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", range(11))
def test_the_class_patch_keeps_every_other_bit(fmt):
    rows = lc.class_records(fmt, 3, seed=fmt)          # the class byte takes every value: every setting of the flag bits
    new = np.random.default_rng(fmt).integers(0, 32 if fmt <= 5 else 256, 256).astype(np.uint8)
    got = rows.copy()
    lw.patch_class_bytes(got, fmt, new)
    col = 15 if fmt <= 5 else 16
    other = np.ones(rows.shape[1], dtype=bool)
    other[col] = False
    assert np.array_equal(got[:, other], rows[:, other])
    if fmt <= 5:
        assert np.array_equal(got[:, col] & 0xE0, rows[:, col] & 0xE0) and np.array_equal(got[:, col] & 31, new)
        assert set((rows[:, col] >> 5).tolist()) == set(range(8))
    else:
        assert np.array_equal(got[:, col], new)
    assert np.array_equal(lc.decode_oracle(got, 256, fmt, rows.shape[1], lc.SCALE, lc.OFFSET)[1], new.astype(np.float64))
    with pytest.raises(ValueError):
        lw.patch_class_bytes(got, fmt, new[:5])
