"""What the K24 tests share (tests/test_voxel_pool_host.py, tests/test_gpu_voxel_pool.py): the rules of sn_voxel_pool
(include/scenenet_hip.h, K24) restated in numpy fp64 over the project's own binning oracle
(tests/binning_cases.py::expected_flat -- pyntcloud is not installed, so its binning is not pinned here, as for K1, K17 and
K18): the quantiser, the integer sums by np.add.at on int64, the decode operation for operation, the order-preserving keys
of the minima and maxima, and the case builders.  No test lives here."""
import math

import numpy as np

import binning_cases as bc
from voxel_classes_cases import bits, cube_tile, key_of, own_desc  # noqa: F401  (shared with the K18 tests)

MEAN, MIN, MAX = 0, 1, 2
TWO32 = 4294967296.0
ALL_ONES = np.uint64(0xFFFFFFFFFFFFFFFF)
CENTROIDS = ([0, 1, 2], [MEAN, MEAN, MEAN])
# mean, min and max of z and of value column 0, then two more of x and y: eight planes
EIGHT = ([2, 2, 2, 3, 3, 3, 0, 1], [MEAN, MIN, MAX, MEAN, MIN, MAX, MIN, MAX])
SPECIAL_VALUES = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 5e-324, -5e-324, 2.2e-308, 1e300, -1e300, -3.5, 0.25, 15.0, 7.0])
VALUE_RANGE = (-4.0, 16.0)


# ---------------------------------------------------------------- the fixed-point mean
def quantiser(lo, hi):
    """(span, inv): span = fl(hi - lo); inv = fl(2^32 / span) if span > 0 and the quotient is finite, else 0."""
    with np.errstate(all="ignore"):
        span = np.float64(hi) - np.float64(lo)
        inv = np.float64(TWO32) / span if span > 0 else np.float64(0.0)
    return span, (inv if span > 0 and np.isfinite(inv) else np.float64(0.0))


def quanta(p, lo, hi):
    """q [n] int64 of the inputs p (none NaN): t = fl(fl(p - lo) * inv); t = t > 0 ? t : 0 (NaN -> 0); t = t < 2^32 ? t :
    2^32; q = rint(t)."""
    _, inv = quantiser(lo, hi)
    p = np.asarray(p, dtype=np.float64)
    with np.errstate(all="ignore"):
        t = (p - np.float64(lo)) * inv
        t = np.where(t > 0.0, t, 0.0)
        t = np.where(t < TWO32, t, TWO32)
    return np.rint(t).astype(np.int64)


def decode_mean(S, n, lo, hi):
    """fl(lo + fl(fl((double)S / (double)n) * step)), step = fl(span / 2^32), for the voxels with n > 0."""
    span, _ = quantiser(lo, hi)
    with np.errstate(all="ignore"):
        step = span / np.float64(TWO32)
        return np.float64(lo) + (S.astype(np.float64) / n.astype(np.float64)) * step


def unkey(k):
    """The fp64 whose order-preserving key is k (the inverse of key_of)."""
    k = np.asarray(k, dtype=np.uint64)
    top = (k >> np.uint64(63)).astype(bool)
    u = np.where(top, k & np.uint64(0x7FFFFFFFFFFFFFFF), ~k)
    return np.ascontiguousarray(u).view(np.float64)


# ---------------------------------------------------------------- the whole call
def expected_pool(desc, dims, tiles, sources, ops, values=None, ranges=None, fill=0.0, own=None):
    """planes [B,P,nz,nx,ny] f64, counts [B,nz,nx,ny] i32, unbinned [B] i64, nan_rows [B] i64 by the rules of the header.
    values: per tile [n, C] (or None); ranges: [C] pairs.  A size-mode descriptor is binned as it stands (own None)."""
    nx, ny, nz = dims
    V, B, P = nx * ny * nz, len(tiles), len(sources)
    used = sorted({s - 3 for s in sources if s >= 3})
    planes = np.empty((B, P, V))
    planes.view(np.int64)[:] = np.array([fill], dtype=np.float64).view(np.int64)[0]
    counts = np.zeros((B, V), dtype=np.int32)
    unbinned, nan_rows = np.zeros(B, dtype=np.int64), np.zeros(B, dtype=np.int64)
    for b, t in enumerate(tiles):
        t = np.asarray(t, dtype=np.float64).reshape(-1, 3)
        if len(t) == 0:
            continue
        flat = bc.expected_flat(desc[b], dims, t, None if own is None else own[b])
        ins = flat >= 0
        unbinned[b] = (~ins).sum()
        val = None if values is None else np.asarray(values[b], dtype=np.float64).reshape(len(t), -1)
        bad = np.zeros(len(t), dtype=bool)
        for c in used:
            bad |= np.isnan(val[:, c])
        nan_rows[b] = (ins & bad).sum()
        part = ins & ~bad
        f = flat[part]
        n = np.bincount(f, minlength=V)
        counts[b] = n
        hit = n > 0
        for p, (s, op) in enumerate(zip(sources, ops)):
            x = t[part, s] if s < 3 else val[part, s - 3]
            if op == MEAN:
                lo, hi = (desc[b][s], desc[b][3 + s]) if s < 3 else ranges[s - 3]
                S = np.zeros(V, dtype=np.int64)
                np.add.at(S, f, quanta(x, lo, hi))
                planes[b, p, hit] = decode_mean(S[hit], n[hit], lo, hi)
            else:
                k = np.full(V, ALL_ONES if op == MIN else np.uint64(0), dtype=np.uint64)
                (np.minimum if op == MIN else np.maximum).at(k, f, key_of(x))
                planes[b, p, hit] = unkey(k[hit])
    return planes.reshape(B, P, nz, nx, ny), counts.reshape(B, nz, nx, ny), unbinned, nan_rows


def fsum_means(desc_row, dims, pts, own_dims=None):
    """Per occupied voxel and axis: (flat index [m], the math.fsum mean of the coordinates clamped to [lo, hi] [m, 3])."""
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    flat = bc.expected_flat(desc_row, dims, pts, own_dims)
    ins = flat >= 0
    f, p = flat[ins], np.clip(pts[ins], desc_row[:3], desc_row[3:6])
    order = np.argsort(f, kind="stable")
    f, p = f[order], p[order]
    cells, start = np.unique(f, return_index=True)
    stop = np.append(start[1:], len(f))
    means = np.array([[math.fsum(p[a:z, k]) / (z - a) for k in range(3)] for a, z in zip(start, stop)]).reshape(-1, 3)
    return cells, means


# ---------------------------------------------------------------- case builders
def special_values(n, rng, nan_share=0.1):
    """n values drawn from SPECIAL_VALUES (NaN, +-inf, +-0.0, denormals among them) and from ordinary numbers inside and
    beyond VALUE_RANGE, more NaN mixed in"""
    v = SPECIAL_VALUES[rng.integers(0, len(SPECIAL_VALUES), n)].copy()
    plain = rng.random(n) < 0.5
    v[plain] = -6.0 + 24.0 * rng.random(int(plain.sum()))
    v[rng.random(n) < nan_share] = np.nan
    return v


def foreign_case(kind, dims, seed=0):
    """(desc [4, len], own | None, tiles): bc.foreign_batch (tiles of 1001 rows, 1 row -- outside its table -- and about n
    rows) and a fourth tile none of whose rows is binned (NaN rows and rows above its table)."""
    desc, own = bc.host_desc(kind, dims, 4)
    tiles, _ = bc.foreign_batch(desc, dims, own, seed=seed)
    hi = desc[3, 3:6]
    nothing = np.concatenate([np.full((2, 3), np.nan), hi + np.array([[1.0, 2.0, 3.0]]) * np.arange(1, 6)[:, None] * 1e3])
    if own is not None:           # (a padded table's cell n_a takes everything above the tile's last edge: only NaN is outside)
        nothing[2:, 1] = np.nan
    return desc, own, tiles + [nothing]
