"""LAS decode (K13): a writer of minimal LAS files, the numpy oracle -- np.frombuffer with the record dtype of the point
format, `X * scale + offset`, the class rule of include/scenenet_hip.h, np.bincount -- and the cases its host and GPU tests
share.  The record layouts are those of the ASPRS LAS 1.4 specification (R15), tables 7-17.  Everything is compared exactly."""
import struct
from fractions import Fraction

import numpy as np

STANDARD_LENGTH = (20, 28, 26, 34, 57, 63, 30, 36, 38, 59, 67)
HEADER_SIZE = (227, 227, 227, 235, 375)          # LAS 1.0 .. 1.4
INT32_EDGES = (-2**31, -1, 0, 1, 2**31 - 1)
SCALE = (0.001, 0.01, 0.0001)
OFFSET = (4.2e6, 500000.0, -12.5)
CONTRACTION = ((0.001, 4.2e6), (0.01, 500000.0))  # (scale, offset) of the two sets the issue measured

_LEGACY = [("X", "<i4"), ("Y", "<i4"), ("Z", "<i4"), ("intensity", "<u2"), ("return_bits", "u1"), ("class_bits", "u1"),
           ("scan_angle_rank", "i1"), ("user_data", "u1"), ("point_source_id", "<u2")]
_MODERN = [("X", "<i4"), ("Y", "<i4"), ("Z", "<i4"), ("intensity", "<u2"), ("return_bits", "u1"), ("flag_bits", "u1"),
           ("classification", "u1"), ("user_data", "u1"), ("scan_angle", "<i2"), ("point_source_id", "<u2"),
           ("gps_time", "<f8")]
_GPS = [("gps_time", "<f8")]
_RGB = [("red", "<u2"), ("green", "<u2"), ("blue", "<u2")]
_NIR = [("nir", "<u2")]
_WAVE = [("wave_index", "u1"), ("wave_offset", "<u8"), ("wave_size", "<u4"), ("wave_location", "<f4"), ("wave_xt", "<f4"),
         ("wave_yt", "<f4"), ("wave_zt", "<f4")]
_FIELDS = (_LEGACY, _LEGACY + _GPS, _LEGACY + _RGB, _LEGACY + _GPS + _RGB, _LEGACY + _GPS + _WAVE,
           _LEGACY + _GPS + _RGB + _WAVE, _MODERN, _MODERN + _RGB, _MODERN + _RGB + _NIR, _MODERN + _WAVE,
           _MODERN + _RGB + _NIR + _WAVE)


def record_dtype(fmt, extra=0):
    """the packed record of point format `fmt` followed by `extra` bytes the format does not define"""
    fields = list(_FIELDS[fmt]) + ([("extra", f"V{extra}")] if extra else [])
    dt = np.dtype(fields)
    assert dt.itemsize == STANDARD_LENGTH[fmt] + extra
    return dt


# ---- the oracle ------------------------------------------------------------------------------------------------------
def decode_oracle(buf, n, fmt, record_length, scale, offset):
    """(pts [n,3] f64, classes [n] f64, hist [256] i64) of the n records at the start of `buf` (bytes / uint8 array)"""
    raw = np.frombuffer(buf, dtype=np.uint8) if isinstance(buf, (bytes, bytearray)) else np.ascontiguousarray(buf).reshape(-1)
    rec = raw[:n * record_length].view(record_dtype(fmt, record_length - STANDARD_LENGTH[fmt]))
    assert rec.shape == (n,)
    pts = np.empty((n, 3), dtype=np.float64)
    for a, name in enumerate("XYZ"):
        pts[:, a] = rec[name] * np.float64(scale[a]) + np.float64(offset[a])   # int32 * f64 -> f64: two roundings
    cls = (rec["class_bits"] & 31) if fmt <= 5 else rec["classification"]
    return pts, cls.astype(np.float64), np.bincount(cls, minlength=256).astype(np.int64)


def fused_result(X, scale, offset):
    """the exactly rounded X * scale + offset (one rounding), what a contracted multiply-add would give"""
    return np.array([float(Fraction(int(x)) * Fraction(float(scale)) + Fraction(float(offset))) for x in X])


def contraction_xs(count=4000, seed=0):
    return np.random.default_rng(seed).integers(-2**31, 2**31, size=count, dtype=np.int64).astype(np.int32)


def contraction_differs(X, scale, offset):
    """how many of X give another double when the product is not rounded on its own"""
    two = X * np.float64(scale) + np.float64(offset)
    return int((fused_result(X, scale, offset) != two).sum())


# ---- records ---------------------------------------------------------------------------------------------------------
def random_records(n, fmt, extra=0, seed=0):
    """[n, record_length] uint8: every byte random -- flag bits, unused fields and the extra bytes too"""
    S = STANDARD_LENGTH[fmt] + extra
    return np.random.default_rng([seed, n, fmt, extra]).integers(0, 256, size=(n, S), dtype=np.uint8)


def set_xyz(rows, X=None, Y=None, Z=None):
    for a, v in enumerate((X, Y, Z)):
        if v is not None:
            rows[:, 4 * a:4 * a + 4] = np.ascontiguousarray(v, dtype="<i4").view(np.uint8).reshape(-1, 4)
    return rows


def set_class_byte(rows, fmt, values):
    rows[:, 15 if fmt <= 5 else 16] = np.asarray(values, dtype=np.uint8)
    return rows


def edge_records(fmt, extra=0, seed=0):
    """125 records: every combination of X, Y, Z over INT32_MIN, -1, 0, 1, INT32_MAX"""
    e = np.array(INT32_EDGES, dtype=np.int64)
    X, Y, Z = (g.reshape(-1) for g in np.meshgrid(e, e, e, indexing="ij"))
    return set_xyz(random_records(125, fmt, extra, seed), X, Y, Z)


def class_records(fmt, extra=0, seed=0):
    """256 records whose class byte takes every value once (formats 0..5: the three flag bits in every setting)"""
    return set_class_byte(random_records(256, fmt, extra, seed), fmt, np.arange(256))


def scan_records(n, fmt, towers, seed=0, extent=400.0, scale=0.01, height=12.0):
    """a synthetic scan for build_data_samples: n ground points of classes 1..9 over extent x extent, plus, per tower
    (cx, cy, count), `count` points of class 15 in a column 2 m wide and `height` high (within DBSCAN's eps = 10 of one another, nearly).  Coordinates are the integers of
    `scale`; every byte that is no coordinate and no class is random."""
    rng = np.random.default_rng([seed, n])
    xs = [rng.uniform(0, extent, n)]
    ys = [rng.uniform(0, extent, n)]
    zs = [rng.uniform(0, 3, n)]
    cls = [rng.integers(1, 10, n)]
    for cx, cy, count in towers:
        xs.append(cx + rng.uniform(-1, 1, count))
        ys.append(cy + rng.uniform(-1, 1, count))
        zs.append(rng.uniform(0, height, count))
        cls.append(np.full(count, 15))
    x, y, z, c = (np.concatenate(v) for v in (xs, ys, zs, cls))
    order = rng.permutation(x.shape[0])
    rows = random_records(x.shape[0], fmt, 0, seed)
    set_xyz(rows, np.rint(x[order] / scale), np.rint(y[order] / scale), np.rint(z[order] / scale))
    return set_class_byte(rows, fmt, c[order] | (0 if fmt > 5 else 0x40))   # (formats 0..5: a flag bit set on top)


# ---- the writer ------------------------------------------------------------------------------------------------------
def las_header(minor, fmt, record_length, n, scale=SCALE, offset=OFFSET, data_offset=None, header_size=None,
               signature=b"LASF", legacy_count=None, format_byte=None, major=1):
    """the public header block of LAS 1.`minor` as bytes; the keyword arguments overwrite single fields, which is how the
    tests build files a reader must refuse"""
    size = HEADER_SIZE[minor] if header_size is None else header_size
    h = bytearray(max(size, HEADER_SIZE[minor]))
    h[0:4] = signature
    h[24], h[25] = major, minor
    h[26:26 + 5] = b"tests"
    struct.pack_into("<HI", h, 94, size, size if data_offset is None else data_offset)
    if legacy_count is None:
        legacy_count = n if ((fmt <= 5 or minor < 4) and n < 2**32) else 0
    struct.pack_into("<BHI", h, 104, fmt if format_byte is None else format_byte, record_length, legacy_count)
    struct.pack_into("<3d", h, 131, *scale)
    struct.pack_into("<3d", h, 155, *offset)
    struct.pack_into("<6d", h, 179, 6.0, 5.0, 4.0, 3.0, 2.0, 1.0)   # the header's own box: a marker, not a true box
    if minor == 4:
        struct.pack_into("<Q", h, 247, n)
    return bytes(h[:max(size, HEADER_SIZE[minor])])


def write_las(path, rows, fmt, minor=2, scale=SCALE, offset=OFFSET, pad=0, trailing=b"", n=None, **header_fields):
    """Writes header, `pad` bytes of variable length records' room (so that the data offset takes any residue), the
    records `rows` [n, record_length] uint8 and `trailing` bytes (LAS 1.4's extended records come last).  `n`: the count
    the header states when it is not rows.shape[0].  Returns the data offset."""
    rows = np.ascontiguousarray(rows, dtype=np.uint8)
    S = rows.shape[1]
    size = header_fields.get("header_size") or HEADER_SIZE[minor]
    data_offset = header_fields.pop("data_offset", max(size, HEADER_SIZE[minor]) + pad)
    head = las_header(minor, fmt, S, rows.shape[0] if n is None else n, scale, offset, data_offset=data_offset,
                      **header_fields)
    with open(path, "wb") as f:
        f.write(head)
        f.write(bytes(max(0, data_offset - len(head))))
        f.write(rows.tobytes())
        f.write(trailing)
    return data_offset
