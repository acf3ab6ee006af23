"""LAS encode (K15): the numpy oracle -- np.rint((x - offset) / scale) per column, the class rule of
include/scenenet_hip.h, the fields assigned to las_cases.record_dtype -- and the cases its host and GPU tests share.
Everything is compared exactly, byte for byte."""
import numpy as np

import las_cases as lc

SERVED = (0, 1, 2, 3, 6, 7, 8)
GPS_FORMATS, RGB_FORMATS = (1, 3, 6, 7, 8), (2, 3, 7, 8)
MAX_RECORD_LENGTH = 80
INT32_MIN, INT32_MAX = -2**31, 2**31 - 1
EMPTY_BOX = (INT32_MAX, INT32_MIN) * 3


# ---- the oracle ------------------------------------------------------------------------------------------------------
def quantise(col, scale, offset):
    """(int32 column, bad mask): rint((x - offset) / scale), two roundings and a rint to even; a NaN quotient -> 0, one
    below -2^31 -> INT32_MIN, one above 2^31 - 1 -> INT32_MAX, all three flagged"""
    with np.errstate(all="ignore"):
        q = (np.asarray(col, dtype=np.float64) - np.float64(offset)) / np.float64(scale)
        nan, low, high = np.isnan(q), q < -2.0**31, q > 2.0**31 - 1
        out = np.rint(np.where(nan | low | high, 0.0, q)).astype(np.int64)
    out[low], out[high], out[nan] = INT32_MIN, INT32_MAX, 0
    return out.astype(np.int32), nan | low | high


def class_bytes(classes, fmt, n):
    """(uint8 column, bad mask): c if c == floor(c) and 0 <= c <= 31 (formats 0..3) | 255 (6..8), else 0 and flagged"""
    if classes is None:
        return np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=bool)
    c = np.asarray(classes, dtype=np.float64)
    with np.errstate(all="ignore"):
        ok = (c == np.floor(c)) & (c >= 0) & (c <= (31 if fmt <= 5 else 255))
    return np.where(ok, c, 0.0).astype(np.uint8), ~ok


def encode_oracle(xyz, classes, intensity, gps, rgb, fmt, extra, scale, offset):
    """(rows [n,S] uint8, box (min X, max X, min Y, max Y, min Z, max Z), hist [256] i64, bad (points, classes))"""
    xyz = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
    n = xyz.shape[0]
    rec = np.zeros(n, dtype=lc.record_dtype(fmt, extra))
    bad_xyz = np.zeros(n, dtype=bool)
    box = []
    for a, name in enumerate("XYZ"):
        rec[name], bad = quantise(xyz[:, a], scale[a], offset[a])
        bad_xyz |= bad
        box += [int(rec[name].min()), int(rec[name].max())] if n else [INT32_MAX, INT32_MIN]
    cls, bad_cls = class_bytes(classes, fmt, n)
    if fmt <= 5:
        rec["return_bits"], rec["class_bits"] = 0x09, cls       # return 1 of 1; the three flag bits zero
    else:
        rec["return_bits"], rec["classification"] = 0x11, cls   # return 1 of 1; byte 15 stays 0
    if intensity is not None:
        rec["intensity"] = np.asarray(intensity).view(np.uint16)
    if gps is not None:
        assert fmt in GPS_FORMATS
        rec["gps_time"] = np.asarray(gps, dtype=np.float64)
    if rgb is not None:
        assert fmt in RGB_FORMATS
        c = np.asarray(rgb).view(np.uint16).reshape(n, 3)
        rec["red"], rec["green"], rec["blue"] = c[:, 0], c[:, 1], c[:, 2]
    rows = rec.view(np.uint8).reshape(n, rec.dtype.itemsize)
    return rows, tuple(box), np.bincount(cls, minlength=256).astype(np.int64), (int(bad_xyz.sum()), int(bad_cls.sum()))


# ---- inputs ----------------------------------------------------------------------------------------------------------
def random_inputs(n, fmt, seed=0, optional=True, scale=lc.SCALE, offset=lc.OFFSET):
    """dict of xyz [n,3] f64 whose integers fill int32 at (scale, offset), and -- with `optional` -- classes the format
    holds, intensity, and gps_time / rgb where the format has them (None otherwise)"""
    rng = np.random.default_rng([seed, n, fmt])
    X = rng.integers(INT32_MIN, INT32_MAX + 1, size=(n, 3), dtype=np.int64)
    xyz = X * np.asarray(scale, dtype=np.float64) + np.asarray(offset, dtype=np.float64)
    xyz += rng.uniform(-0.4, 0.4, size=(n, 3)) * np.asarray(scale)          # off the grid, away from the ties
    out = {"xyz": xyz, "classes": None, "intensity": None, "gps": None, "rgb": None}
    if optional:
        out["classes"] = rng.integers(0, 32 if fmt <= 5 else 256, n).astype(np.float64)
        out["intensity"] = rng.integers(0, 65536, n).astype(np.uint16)
        if fmt in GPS_FORMATS:
            out["gps"] = rng.integers(0, 2**63, n, dtype=np.int64).view(np.float64).copy()   # any bit pattern: a bit copy
        if fmt in RGB_FORMATS:
            out["rgb"] = rng.integers(0, 65536, (n, 3)).astype(np.uint16)
    return out


def oracle_of(inp, fmt, extra=0, scale=lc.SCALE, offset=lc.OFFSET):
    return encode_oracle(inp["xyz"], inp["classes"], inp["intensity"], inp["gps"], inp["rgb"], fmt, extra, scale, offset)


def tie_inputs(scale, half_range=200_000):
    """x = (k + 0.5) * scale for k in -half_range .. half_range - 1, offset 0: quotients at or next to a tie"""
    k = np.arange(-half_range, half_range, dtype=np.float64)
    return (k + 0.5) * np.float64(scale)


def reciprocal_differs(x, scale):
    """how many of x quantise to another integer when the division is replaced by a product with 1 / scale"""
    s = np.float64(scale)
    return int((np.rint(x / s) != np.rint(x * (np.float64(1.0) / s))).sum())


def rounding_xyz(scale=0.001):
    """[m,3] f64 for offset 0: the tie set and its negatives, +-0.0, NaN, +-inf, quotients just inside and just outside
    int32 -- in every column in turn, so that `bad` has to count points, not coordinates"""
    t = tie_inputs(scale, 20_000)
    s = np.float64(scale)
    inside = [INT32_MAX * s, INT32_MIN * s, (INT32_MAX - 0.5) * s, (INT32_MIN + 0.5) * s, np.nextafter(2.0**31 - 1, 0) * s]
    outside = [(2.0**31) * s, (INT32_MIN - 1.0) * s, 1e300, -1e300, (INT32_MAX + 0.75) * s, (INT32_MIN - 0.75) * s]
    special = np.array([0.0, -0.0, np.nan, np.inf, -np.inf] + inside + outside, dtype=np.float64)
    col = np.concatenate([t, -t, special])
    m = col.shape[0]
    xyz = np.stack([col, np.roll(col, 7), np.roll(col, m // 2)], axis=1)
    # three points whose coordinates are ALL out of range: each counts once
    return np.concatenate([xyz, np.array([[np.nan, np.inf, -np.inf], [1e300, 1e300, np.nan], [-1e300, np.nan, np.nan]])])


CLASS_VALUES = (0.0, 15.0, 31.0, 32.0, 80.0, 255.0, 256.0, -1.0, 15.5, float("nan"), -0.0, float("inf"))
