"""Nearest neighbours (K21): the numpy oracle -- brute force over all pairs in the literal formula of
include/scenenet_hip.h -- the host restatement of avg_dist_points over it, and the point sets the host and GPU tests
share (those of dbscan_cases.py).  Everything is compared exactly unless a test says otherwise.  Sets stay at m <= 3000."""
import functools
import math
import warnings

import numpy as np

from dbscan_cases import (ORIGIN, SEAM_BOUNDS, SEAM_EPS, SEAM_LO, blobs_case, contraction_case, nonfinite_case,  # noqa: F401
                          rim_case, seam_case, small_cloud, squared_distances)

KS = (1, 3, 4, 5, 8, 16)          # on and between the kernel's instantiations 1, 4, 8, 16
BLOB_RADIUS = (6.0, 2.5, 2.5, 1.6)


# ---- the oracle ------------------------------------------------------------------------------------------------------
def knn_oracle(P, radius, k, exclude_zero=False):
    """(d2 [m,k] f64, found [m] i32, mean_dist [m] f64, index [m,k] i64) of ONE tile: candidates q != p with
    (dx*dx + dy*dy) + dz*dz <= radius*radius (and > 0 with exclude_zero), the k first by (d2, index)"""
    m = P.shape[0]
    d2 = np.full((m, k), np.inf)
    index = np.full((m, k), -1, dtype=np.int64)
    found = np.zeros(m, dtype=np.int32)
    mean = np.full(m, np.nan)
    r2 = radius * radius
    for r0 in range(0, m, 512):
        rows = slice(r0, min(r0 + 512, m))
        with np.errstate(all="ignore"):
            D = squared_distances(P, rows)
            mask = D <= r2
        mask[np.arange(rows.stop - r0), np.arange(r0, rows.stop)] = False       # the diagonal: q != p by row index
        if exclude_zero:
            mask &= D > 0
        found[rows] = mask.sum(axis=1)
        for i in range(rows.stop - r0):
            cand = np.flatnonzero(mask[i])
            order = cand[np.lexsort((cand, D[i, cand]))][:k]
            c = len(order)
            d2[r0 + i, :c] = D[i, order]
            index[r0 + i, :c] = order
            if c:
                s = np.sqrt(D[i, order])
                acc = s[0]
                for v in s[1:]:
                    acc = acc + v                                               # ascending, one rounding each
                mean[r0 + i] = acc / np.float64(c)
    return d2, found, mean, index


def batch_oracle(tiles, radius, k, exclude_zero=False):
    """the oracle of every tile, packed: indices are packed row indices"""
    outs, at = [], 0
    for P in tiles:
        if len(P) == 0:
            continue
        d2, found, mean, index = knn_oracle(P, radius, k, exclude_zero)
        outs.append((d2, found, mean, np.where(index >= 0, index + at, -1)))
        at += len(P)
    return tuple(np.concatenate([o[j] for o in outs]) for j in range(4))


def tile_stats_oracle(found, mean, k):
    """(n_valid, n_full, sum, sum_sq, max) of one tile with math.fsum; max is -inf without a valid row"""
    valid = found >= 1
    v = mean[valid]
    return (int(valid.sum()), int((found >= k).sum()), math.fsum(v.tolist()), math.fsum((v * v).tolist()),
            float(v.max()) if v.size else -np.inf)


def spacing_oracle(found, mean, k):
    """(mean, population std) as sna.point_spacing forms them from the statistics"""
    n, _, s, sq, _ = tile_stats_oracle(found, mean, k)
    if n == 0:
        return np.nan, np.nan
    mu = s / n
    return mu, math.sqrt(max(sq / n - mu * mu, 0.0))


@functools.lru_cache(maxsize=None)
def oracle_of_blobs(which, k, exclude_zero=False):
    return knn_oracle(blobs_case(which)[0], BLOB_RADIUS[which], k, exclude_zero)


def noisy_blobs(which=2, share=0.05, seed=41):
    """blobs_case(which) with `share` uniform noise in a box three times its extent appended and the rows shuffled"""
    P = blobs_case(which)[0]
    rng = np.random.default_rng(seed)
    lo, hi = P.min(axis=0), P.max(axis=0)
    n = int(len(P) * share)
    noise = lo - (hi - lo) + rng.random((n, 3)) * 3.0 * (hi - lo)
    Q = np.concatenate([P, noise])
    return np.ascontiguousarray(Q[rng.permutation(len(Q))])


# ---- avg_dist_points -------------------------------------------------------------------------------------------------
def running_means(table, num_dists):
    """the reference's avgs from each row's num_dists smallest positive distances (+inf where fewer): its list after
    point i holds the positive distances of the points 0..i, and np.sort(dists)[:num_dists] of that list lies inside the
    union of those rows' own num_dists smallest"""
    avgs, dists = [], np.empty(0)
    for row in table:
        dists = np.sort(np.concatenate([dists, row[np.isfinite(row)]]))[:num_dists]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            avgs.append(np.mean(dists))
    return np.array(avgs)


def avg_dist_points_host(xyz, accuracy, num_dists):
    """avg_dist_points restated over the oracle (brute force: the radius reaches every pair)"""
    view = xyz[:round(len(xyz) * accuracy)]
    span = float(np.linalg.norm(view.max(axis=0) - view.min(axis=0)))
    d2 = knn_oracle(view, max(span, 1e-9) * (1.0 + 1e-6), num_dists, exclude_zero=True)[0]
    return float(np.mean(running_means(np.sqrt(d2), num_dists)))


def avg_dist_bound(m, num_dists):
    """relative: one rounding per distance (np.linalg.norm against sqrt of the literal sum) and those of the two means"""
    return (num_dists + m + 4) * 2.0 ** -53


def golden_clouds():
    """[(name, xyz, accuracy, num_dists)]: six small clouds at UTM offsets"""
    rng = np.random.default_rng(77)
    out = []
    for name, m, acc, nd, spread in (("plain25", 25, 1.0, 1, 6.0), ("half80", 80, 0.5, 3, 9.0), ("five60", 60, 1.0, 5, 4.0),
                                     ("sixteen48", 48, 1.0, 16, 7.0)):
        out.append((name, np.ascontiguousarray(ORIGIN + rng.random((m, 3)) * spread), acc, nd))
    P = ORIGIN + rng.random((40, 3)) * 5.0
    P[17] = P[3]                                    # a duplicated point: its distance 0 is dropped like the point's own
    out.append(("duplicate40", np.ascontiguousarray(P), 1.0, 3))
    # num_dists beyond the positive distances of the first rows: 3 points give 4 entries after row 1, 6 after row 2 < 16
    out.append(("short30", np.ascontiguousarray(ORIGIN + rng.random((30, 3)) * 3.0), 0.1, 16))
    return out
