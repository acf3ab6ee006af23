"""Region census (K12): the numpy oracle -- crops_cases.region_mask for membership, then len, np.isnan, min / max and the
literal range test --, the case generators its host and GPU tests share, and numpy restatements of what the three sample
builders compute, written independently with the reference's deciding arithmetic (utils/pcd_processing.py:742-762 crop_ground_samples, pinned by the golden
fixture scan_census.npz; core/datasets/semKITTI.py:37-88 build_pole_samples and :91-158 crop_tower_samples under
build_pole_radius_samples, pinned by source reading only: semKITTI.py cannot be imported).  Everything is compared
exactly: integers as they are, fp64 as int64 views."""
import numpy as np

import crops_cases as cc
import dbscan_cases as dc

TOWER = 15               # POWER_LINE_SUPPORT_TOWER
POLE = 80


# ---- the oracle ------------------------------------------------------------------------------------------------------
def _signed_min_max(l):
    """(min, max) of a non-empty array without NaN, in the order that puts -0.0 below +0.0"""
    lo, hi = l.min(), l.max()
    zeros = l[l == 0]
    if lo == 0:
        lo = -0.0 if np.signbit(zeros).any() else 0.0
    if hi == 0:
        hi = 0.0 if (~np.signbit(zeros)).any() else -0.0
    return lo, hi


def census_oracle(pts, labels, regions, kinds, watch):
    """(counts [K, 2 + C] i64, label_range [K,2] f64 | None without labels)"""
    K = regions.shape[0]
    kinds = np.zeros(K, dtype=np.int32) if kinds is None else kinds
    watch = np.zeros((0, 2)) if watch is None else np.asarray(watch, dtype=np.float64).reshape(-1, 2)
    C = watch.shape[0]
    counts = np.zeros((K, 2 + C), dtype=np.int64)
    rng = None if labels is None else np.empty((K, 2), dtype=np.float64)
    for k in range(K):
        mask = cc.region_mask(pts, regions[k], int(kinds[k]))
        counts[k, 0] = len(pts[mask])
        if labels is None:
            continue
        l = labels[mask]
        counts[k, 1] = np.isnan(l).sum()
        with np.errstate(all="ignore"):
            for c in range(C):
                counts[k, 2 + c] = ((watch[c, 0] <= l) & (l <= watch[c, 1])).sum()
        l = l[~np.isnan(l)]
        rng[k] = _signed_min_max(l) if len(l) else (np.inf, -np.inf)
    return counts, rng


def distinct_ge2(n, n_nan, lo, hi):
    """the predicate RegionCensus.distinct_ge2 states, on host values"""
    return bool(lo < hi or (n_nan > 0 and n_nan < n))


# ---- cases -----------------------------------------------------------------------------------------------------------
ODD_LABELS = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 5e-324, -5e-324, 2.2250738585072014e-308, 15.0, 15.999999999999998,
                       16.0, 80.0, -3.0, 1e300])


def odd_labels(n, seed):
    """labels drawn from ODD_LABELS and the ordinary classes: NaN, +-inf, +-0.0 and denormals in every region of a size"""
    rng = np.random.default_rng(seed)
    return np.where(rng.random(n) < 0.5, rng.choice(ODD_LABELS, n), rng.choice(np.array([0.0, 2.0, 15.0, 16.0, 80.0]), n))


def watch_rows(C, seed=0):
    """C ranges: equalities, truncation ranges, an infinite range, a reversed (empty) one, +-0.0, and NaN bounds"""
    rows = [[15.0, 15.0], [15.0, np.nextafter(16.0, -np.inf)], [-np.inf, np.inf], [0.0, -0.0], [np.nan, 80.0], [80.0, np.nan],
            [16.0, 2.0], [-5e-324, 5e-324], [np.inf, np.inf], [np.nextafter(-1.0, 0.0), np.nextafter(1.0, 0.0)], [2.0, 16.0],
            [80.0, 80.0], [-np.inf, -np.inf], [np.nan, np.nan], [1e300, np.inf], [-3.0, -3.0]]
    assert len(rows) == 16
    return np.array(rows[:C], dtype=np.float64).reshape(-1, 2)


def late_chunk_case(chunk):
    """(pts, labels, regions, kinds): 3 * chunk + 17 points far from region 0 except a few in the LAST chunk, and region 1
    holds nothing at all: the slots of the chunks that do not reach a region must read 0, not what the workspace held"""
    rng = np.random.default_rng(61)
    n = 3 * chunk + 17
    pts = cc.ORIGIN + rng.random((n, 3)) * np.array([40.0, 40.0, 10.0])
    pts[3 * chunk + 2:3 * chunk + 9, :2] = cc.ORIGIN[:2] + np.array([500.0, 500.0]) + rng.random((7, 2))
    labels = odd_labels(n, 62)
    regions = np.array([[cc.ORIGIN[0] + 500.5, cc.ORIGIN[1] + 500.5, 3.0, 0.0], [cc.ORIGIN[0] - 900.0, cc.ORIGIN[1], 5.0, 0.0],
                        [cc.ORIGIN[0] + 499.0, cc.ORIGIN[1] + 499.0, cc.ORIGIN[0] + 502.0, cc.ORIGIN[1] + 502.0]])
    return pts, labels, regions, np.array([0, 0, 1], dtype=np.int32)


SHARDS = 8          # sn_crop_census spreads its workgroups over this many copies of the workspace (workgroup b: b % 8)


def shard_case(chunk):
    """(pts, labels, regions, kinds) with 19 * chunk + 17 points, 20 workgroups: every shard of the workspace is shared by
    two or three workgroups, so counts are added onto non-zero slots and maxima meet values that are already there.
    Regions: a box that holds every point, three overlapping discs over the middle of the cloud (members in every
    chunk), a disc that holds nothing, and a far box whose members lie in the chunks 1, 9 and 17 alone -- one shard --
    with its smallest label in chunk 9, its largest in chunk 1 and NaNs in chunk 17."""
    rng = np.random.default_rng(81)
    n = 19 * chunk + 17
    pts = cc.ORIGIN + rng.random((n, 3)) * np.array([60.0, 60.0, 40.0])
    labels = odd_labels(n, 82)
    far = cc.ORIGIN[:2] + np.array([900.0, -700.0])
    for c, values in ((1, [5.0, 1e300, 7.0]), (9, [6.0, -1e300, 80.0, 15.5]), (17, [np.nan, 15.0, np.nan])):
        at = c * chunk + 100 + 7 * np.arange(len(values))
        pts[at, :2] = far + rng.random((len(values), 2))
        labels[at] = values
    mid = cc.ORIGIN[:2] + 30.0
    regions = np.array([[-np.inf, -np.inf, np.inf, np.inf], [mid[0], mid[1], 25.0, 0.0], [mid[0] + 8.0, mid[1] - 5.0, 22.0, 0.0],
                        [mid[0] - 6.0, mid[1] + 9.0, 28.0, 0.0], [mid[0], mid[1] + 5000.0, 10.0, 0.0],
                        [far[0] - 1.0, far[1] - 1.0, far[0] + 2.0, far[1] + 2.0]])
    return pts, labels, regions, np.array([1, 0, 0, 0, 0, 1], dtype=np.int32)


# ---- restatements of the reference's builders ------------------------------------------------------------------------
# Written from the builders' behaviour, with the arithmetic that decides a result kept as the reference has it: the slab
# width is the Python int `step`, the upper bound is the fp64 sum start + step, both ends are inclusive, the starts are
# np.linspace(min, max, step), and a class is compared after astype(int) where the reference does so.
def _slabs(values, divisor):
    """(starts, step) of the slabs along one coordinate column"""
    lo, hi = values.min(), values.max()
    step = int((hi - lo) / divisor)
    return np.linspace(lo, hi, step), step


def ground_samples_restated(xyz, classes):
    """what utils/pcd_processing.py:742-762 returns: per slab along x with more than 300 points, at least two distinct
    classes and no class that is 15 after astype(int), the rows (x, y, z, class as int) -- and each sample's mask"""
    samples, masks = [], []
    starts, step = _slabs(xyz[:, 0], 100)
    for start in starts:
        inside = (xyz[:, 0] >= start) & (xyz[:, 0] <= start + step)
        cls = classes[inside]
        as_int = cls.astype(int)
        if inside.sum() <= 300 or len(np.unique(cls)) < 2 or (as_int == TOWER).any():
            continue
        samples.append(np.column_stack([xyz[inside], as_int.astype(np.float64)]))
        masks.append(inside)
    return samples, masks


def pole_slabs_restated(xyz, gt, pole_label=POLE):
    """what the loop of semKITTI.py:69-88 saves for one scan: per slab along the axis of the largest extent (ten steps'
    worth of width) with at least five labels equal to pole_label, the rows (x, y, z, label)"""
    extent = xyz.max(axis=0) - xyz.min(axis=0)
    idx = int(np.argmax(extent))
    samples = []
    starts, step = _slabs(xyz[:, idx], 10)
    for start in starts:
        inside = (xyz[:, idx] >= start) & (xyz[:, idx] <= start + step)
        if np.isin(gt[inside], [pole_label]).sum() >= 5:
            samples.append(np.column_stack([xyz[inside], gt[inside]]))
    return samples


def pole_radius_restated(xyz, gt, pole_label=POLE, eps=5, min_points=10, radius=5):
    """what semKITTI.py:91-103 and the gate and filter of :142-153 keep for one scan: per cluster of the pole points
    (DBSCAN oracle of dbscan_cases; the reference asks open3d), in id order, the disc of `radius` around the cluster's mean
    in the plane (crops_cases.disc_mask), rows (x, y, z, class as int), kept with at least five classes equal to
    pole_label after astype(int)"""
    if not (gt == pole_label).any():
        return []
    poles = xyz[np.isin(gt, [pole_label])]
    cluster, n_clusters, _, _ = dc.dbscan_oracle(poles, eps, min_points)
    samples = []
    for t in range(n_clusters):
        centre = poles[cluster == t].mean(axis=0)
        inside = cc.disc_mask(xyz, centre[:2], radius)
        as_int = gt[inside].astype(int)
        if (as_int == pole_label).sum() >= 5:
            samples.append(np.column_stack([xyz[inside], as_int.astype(np.float64)]))
    return samples


def kitti_scan(axis, seed=0, poles=True):
    """(xyz, gt): a scan whose largest extent, 30 m, lies along `axis` (the others span 12 m): step = 3, slabs of 3 m
    starting at min, the middle and max.  Coordinates on a 2^-10 lattice and poles of 16 points: every mean of a pole is exact, however it is summed.  With poles:
    slab 0 holds a pole of 16 points (accepted), the middle slab a pole of 16 and, away from it, 4 loose pole points
    (accepted; the loose ones are DBSCAN noise), and 4 pole points sit outside every slab; the last slab holds the
    extreme point alone (rejected)."""
    rng = np.random.default_rng(300 + 10 * axis + seed)
    lat = lambda lo, hi, size: np.round(rng.uniform(lo, hi, size) * 1024.0) / 1024.0   # noqa: E731
    other = [a for a in range(3) if a != axis]
    n = 900
    xyz = np.empty((n, 3))
    xyz[:, axis] = lat(0.0, 29.0, n)
    for a in other:
        xyz[:, a] = lat(-6.0, 6.0, n)
    xyz[0, axis], xyz[1, axis] = 0.0, 30.0
    xyz[2, other[0]], xyz[3, other[0]] = -6.0, 6.0
    gt = rng.choice(np.array([40.0, 70.0, 81.0, 80.5]), n)
    if poles:
        def pole(count, along, c0, c1):
            p = np.empty((count, 3))
            p[:, axis] = along + lat(-0.4, 0.4, count)
            p[:, other[0]] = c0 + lat(-0.4, 0.4, count)
            p[:, other[1]] = c1 + lat(-0.4, 0.4, count)
            return p
        extra = [pole(16, 1.5, -2.0, 1.0), pole(16, 16.0, 3.0, -3.0)]
        loose = np.empty((4, 3))
        loose[:, axis] = [15.2, 15.9, 16.8, 17.6]
        loose[:, other[0]] = [-5.5, -5.0, -5.5, -5.0]
        loose[:, other[1]] = [5.5, 5.0, -5.5, 5.0]
        away = pole(4, 24.0, 0.0, 0.0)
        extra += [loose, away]
        xyz = np.vstack([xyz] + extra)
        gt = np.concatenate([gt, np.full(sum(len(e) for e in extra), 80.0)])
    order = rng.permutation(len(xyz))
    return np.ascontiguousarray(xyz[order]), np.ascontiguousarray(gt[order])
