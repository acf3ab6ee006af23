"""Helper of the tower-score tests (not collected): the oracle of sn_tower_centroids / sn_tower_match (K11,
include/scenenet_hip.h) and builders that fabricate statistics tables directly -- the kernels read nothing else, so edge
cases need no DBSCAN run.

The oracle calls the project's host mirrors so that they stay the single statement of the rule: sna.filter_towers with
each tower given as the two rows [lo * s, hi * s] and centroids = (sum / n) * s, sna.aggregate_centroids for the
aggregation, a literal numpy restatement of compute_euc_dists' matching loop (utils/observer_utils.py:456-463) and a Python
loop for the totals."""
import math

import numpy as np

import scene_net_amd as sna

NSTAT = 12
NTOTAL = 8
TOTAL_NAMES = ("tiles", "tiles_skipped", "gt_towers", "proposals", "hits", "misses", "false_proposals", "reserved")


def plane_of(height_axis):
    return [a for a in range(3) if a != height_axis]


def size_of(voxel_size):
    return np.ones(3) if voxel_size is None else np.array([float(v) for v in voxel_size], dtype=np.float64)


# --------------------------------------------------------------------------- fabricated tables
def row(n, sums, lo=None, hi=None):
    """one statistics row: n voxels with the index sums `sums`; the box defaults to the centroid's floor / ceiling"""
    sums = [int(v) for v in sums]
    lo = [v // n for v in sums] if lo is None else [int(v) for v in lo]
    hi = [-((-v) // n) for v in sums] if hi is None else [int(v) for v in hi]
    return [int(n), int(n), *sums, *lo, *hi, 0]


def at(c, n=1, lo=None, hi=None):
    """a row whose centroid is c (three numbers with c * n integral)"""
    sums = [round(float(v) * n) for v in c]
    assert all(s / n == float(v) for s, v in zip(sums, c)), "centroid not representable with this count"
    return row(n, sums, lo, hi)


def table(tiles, K, n_towers=None):
    """tiles: per tile a list of rows (at most K are stored) -> (stats int64 [B, K, NSTAT], n_towers int32 [B]);
    n_towers defaults to the tiles' row counts"""
    B = len(tiles)
    st = np.zeros((B, K, NSTAT), dtype=np.int64)
    for b, rows in enumerate(tiles):
        for i, r in enumerate(rows[:K]):
            st[b, i] = r
    nt = np.array([len(t) for t in tiles] if n_towers is None else n_towers, dtype=np.int32)
    return st, nt


def random_rows(count, seed, extent=None, holes=0):
    """`count` rows with fractional centroids (denominators 1..12) spread so that a row has a neighbour or two within 1.5
    in the plane, random boxes around them; `holes` of them with n_voxels = 0"""
    rng = np.random.default_rng(seed)
    extent = max(3, int(math.sqrt(count) * 2)) if extent is None else extent
    rows = []
    for _ in range(count):
        n = int(rng.integers(1, 13))
        sums = rng.integers(0, extent * n + 1, size=3)
        lo = sums // n - rng.integers(0, 4, size=3)
        hi = -((-sums) // n) + rng.integers(0, 12, size=3)
        rows.append(row(n, sums, np.maximum(lo, 0), hi))
    for i in rng.choice(count, size=min(holes, count), replace=False):
        rows[int(i)] = [0] * NSTAT
    return rows


# --------------------------------------------------------------------------- the oracle
def coordinates(stats_tile, n_towers, voxel_size=None):
    """(present bool [K], centroids [K, 3], lo * s [K, 3], hi * s [K, 3]) by the header's coordinate rule"""
    s = size_of(voxel_size)
    K = stats_tile.shape[0]
    present = (np.arange(K) < min(max(int(n_towers), 0), K)) & (stats_tile[:, 0] > 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        cents = (stats_tile[:, 2:5].astype(np.float64) / stats_tile[:, 0:1].astype(np.float64)) * s
    return present, cents, stats_tile[:, 5:8].astype(np.float64) * s, stats_tile[:, 8:11].astype(np.float64) * s


def centroids_oracle(stats, n_towers, height_axis=0, voxel_size=None, center=None, apply_filter=True, threshold=1.75,
                     tower_height=14.0, radius=15.0, min_euc=1.5):
    """-> dict(keep uint8 [B, K], planar [B, K, 2], agg [B, K, 2], n_agg int32 [B], status int32 [B])"""
    B, K = stats.shape[:2]
    plane = plane_of(height_axis)
    keep = np.zeros((B, K), dtype=np.uint8)
    planar = np.full((B, K, 2), np.nan)
    agg = np.full((B, K, 2), np.nan)
    n_agg = np.zeros(B, dtype=np.int32)
    status = (n_towers > K).astype(np.int32)
    for b in range(B):
        present, cents, lo, hi = coordinates(stats[b], n_towers[b], voxel_size)
        planar[b, present] = cents[present][:, plane]
        for i in np.flatnonzero(present):
            if apply_filter:
                kept, _ = sna.filter_towers([np.stack([lo[i], hi[i]])], cents[i:i + 1], float(threshold), center,
                                            height_axis=height_axis, tower_height=float(tower_height), radius=float(radius))
                keep[b, i] = len(kept)
            else:
                keep[b, i] = 1
        rows = sna.aggregate_centroids(cents[keep[b] == 1], height_axis=height_axis, min_euc=min_euc)
        n_agg[b] = len(rows)
        agg[b, :len(rows)] = rows
    return dict(keep=keep, planar=planar, agg=agg, n_agg=n_agg, status=status)


def match_oracle(agg, n_agg, status_pred, gt_stats, gt_n_towers, height_axis=0, voxel_size=None, hit_dist=math.inf):
    """-> dict(match int32 [B, Kg], dist [B, Kg], gt_planar [B, Kg, 2], totals int64 [NTOTAL], hit_dists: per tile the
    hits' distances in row order (skipped tiles: none))"""
    B, Kg = gt_stats.shape[:2]
    plane = plane_of(height_axis)
    match = np.full((B, Kg), -1, dtype=np.int32)
    dist = np.full((B, Kg), np.nan)
    gt_planar = np.full((B, Kg, 2), np.nan)
    totals = dict.fromkeys(TOTAL_NAMES, 0)
    hit_dists = []
    for b in range(B):
        present, cents, _, _ = coordinates(gt_stats[b], gt_n_towers[b], voxel_size)
        gt_centroids = cents[present][:, plane]
        gt_planar[b, present] = gt_centroids
        vxg_centroids = agg[b, :n_agg[b]]
        if len(vxg_centroids) > 0:
            out = []
            for gt_c in gt_centroids:                     # the reference's loop, literally
                gt_full = np.full_like(vxg_centroids, gt_c)
                euc_dists = np.linalg.norm(gt_full - vxg_centroids, axis=1)
                argmin = np.argmin(euc_dists)
                out.append((argmin, euc_dists[argmin]))
        else:
            out = [(-1, 0.0) for _ in gt_centroids]
        for k, (m, d) in zip(np.flatnonzero(present), out):
            match[b, k], dist[b, k] = m, d
        if (status_pred[b] & 1) or gt_n_towers[b] > Kg:
            totals["tiles_skipped"] += 1
            hit_dists.append([])
            continue
        hits = [(m, d) for m, d in out if m >= 0 and d <= hit_dist]
        totals["tiles"] += 1
        totals["gt_towers"] += len(out)
        totals["proposals"] += int(n_agg[b])
        totals["hits"] += len(hits)
        totals["misses"] += len(out) - len(hits)
        totals["false_proposals"] += int(n_agg[b]) - len({int(m) for m, _ in hits})
        hit_dists.append([float(d) for _, d in hits])
    return dict(match=match, dist=dist, gt_planar=gt_planar,
                totals=np.array([totals[n] for n in TOTAL_NAMES], dtype=np.int64), hit_dists=hit_dists)


def same_bits(a, b):
    """equal shapes, dtypes and bit patterns (fp64 compared as int64: NaN rows and signed zeros count)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == np.float64:
        return np.array_equal(a.view(np.int64), b.view(np.int64))
    return np.array_equal(a, b)


def dist_total_bound(hit_dists):
    """(math.fsum of all hits' distances, the bound of any summation order: hits * 2^-53 * sum)"""
    flat = [d for tile in hit_dists for d in tile]
    total = math.fsum(flat)
    return total, len(flat) * 2.0 ** -53 * total
