"""Helper of the tower-proposal tests (not collected): a plain-numpy oracle of sn_tower_proposals' definition
(include/scenenet_hip.h, K8) and the case builders the host and GPU tests share.  No sklearn, no scipy."""
import math

import numpy as np

STAT_NAMES = ("n_voxels", "n_core", "sum_i0", "sum_i1", "sum_i2", "min_i0", "min_i1", "min_i2", "max_i0", "max_i1",
              "max_i2", "first_core_index")
NSTAT = len(STAT_NAMES)


def stencil_offsets(eps, voxel_size=None):
    """[(d0, d1, d2)] with (d0 s0)^2 + (d1 s1)^2 + (d2 s2)^2 <= eps^2, in fp64 in exactly this form, ascending."""
    s = (1.0, 1.0, 1.0) if voxel_size is None else tuple(float(v) for v in voxel_size)
    eps = float(eps)
    r = [int(math.floor(eps / v)) + 1 for v in s]
    out = []
    for d0 in range(-r[0], r[0] + 1):
        for d1 in range(-r[1], r[1] + 1):
            for d2 in range(-r[2], r[2] + 1):
                a, b, c = d0 * s[0], d1 * s[1], d2 * s[2]
                if a * a + b * b + c * c <= eps * eps:
                    out.append((d0, d1, d2))
    return out


def rows_to_offsets(rows):
    """the C entry's rows (d0, d1, half-width) -> the offset list, ascending"""
    return [(int(d0), int(d1), d2) for d0, d1, hw in rows for d2 in range(-int(hw), int(hw) + 1)]


def dbscan_grid(positive, eps, min_points, voxel_size=None, max_towers=None):
    """The definition on one tile.  positive: bool [n0, n1, n2].  Returns (labels int32 [n0, n1, n2], K, stats int64
    [max_towers or K, NSTAT], core bool [n0, n1, n2])."""
    positive = np.asarray(positive, dtype=bool)
    shape = positive.shape
    offs = np.array(stencil_offsets(eps, voxel_size), dtype=np.int64)
    R = int(np.abs(offs).max()) if len(offs) else 0
    pad = np.pad(positive, R)
    pts = np.argwhere(positive)                           # memory order
    cnt = np.zeros(len(pts), dtype=np.int64)
    for o in offs:
        q = pts + o + R
        cnt += pad[q[:, 0], q[:, 1], q[:, 2]]
    is_core = cnt >= min_points
    cores = pts[is_core]
    nc = len(cores)
    core_grid = np.zeros(shape, dtype=bool)
    core_grid[cores[:, 0], cores[:, 1], cores[:, 2]] = True
    cidx = np.full(tuple(n + 2 * R for n in shape), -1, dtype=np.int64)
    cidx[cores[:, 0] + R, cores[:, 1] + R, cores[:, 2] + R] = np.arange(nc)
    # connected components of the cores: hook to the smaller label and jump pointers until nothing changes
    pa, pb = [], []
    for o in offs:
        if tuple(o) <= (0, 0, 0):
            continue
        q = cores + o + R
        nb = cidx[q[:, 0], q[:, 1], q[:, 2]]
        m = nb >= 0
        pa.append(np.flatnonzero(m))
        pb.append(nb[m])
    a = np.concatenate(pa) if pa else np.zeros(0, dtype=np.int64)
    b = np.concatenate(pb) if pb else np.zeros(0, dtype=np.int64)
    lab = np.arange(nc)
    while True:
        la, lb = lab[a], lab[b]
        m = np.minimum(la, lb)
        new = lab.copy()
        for tgt in (la, lb, a, b):
            np.minimum.at(new, tgt, m)
        while True:
            nn = new[new]
            if np.array_equal(nn, new):
                break
            new = nn
        if np.array_equal(new, lab):
            break
        lab = new
    roots = np.unique(lab)                                # ascending smallest core voxel
    K = len(roots)
    cid = np.searchsorted(roots, lab)
    labels = np.full(shape, -1, dtype=np.int32)
    labels[cores[:, 0], cores[:, 1], cores[:, 2]] = cid
    # borders: the smallest id among the cores in the stencil
    cid_pad = np.full(cidx.shape, np.iinfo(np.int64).max, dtype=np.int64)
    cid_pad[cores[:, 0] + R, cores[:, 1] + R, cores[:, 2] + R] = cid
    rest = pts[~is_core]
    best = np.full(len(rest), np.iinfo(np.int64).max, dtype=np.int64)
    for o in offs:
        q = rest + o + R
        best = np.minimum(best, cid_pad[q[:, 0], q[:, 1], q[:, 2]])
    hit = best != np.iinfo(np.int64).max
    labels[rest[hit, 0], rest[hit, 1], rest[hit, 2]] = best[hit]
    rows = K if max_towers is None else max_towers
    return labels, K, stats_of(labels, core_grid, rows), core_grid


def stats_of(labels, core_grid, rows):
    """stats [rows, NSTAT] int64 of a labelled tile (rows of absent clusters zero)."""
    st = np.zeros((rows, NSTAT), dtype=np.int64)
    n2 = labels.shape[2]
    n1 = labels.shape[1]
    idx = np.argwhere(labels >= 0)
    ids = labels[labels >= 0]
    for k in range(min(rows, int(ids.max()) + 1 if len(ids) else 0)):
        p = idx[ids == k]
        c = p[core_grid[p[:, 0], p[:, 1], p[:, 2]]]
        first = c[0]
        st[k] = [len(p), len(c), *p.sum(axis=0), *p.min(axis=0), *p.max(axis=0), (first[0] * n1 + first[1]) * n2 + first[2]]
    return st


def dbscan_batch(positive, eps, min_points, voxel_size=None, max_towers=64):
    """positive bool [B, n0, n1, n2] -> (labels [B, ...] int32, n_towers [B] int32, stats [B, max_towers, NSTAT] int64)"""
    out = [dbscan_grid(p, eps, min_points, voxel_size, max_towers) for p in positive]
    return (np.stack([o[0] for o in out]), np.array([o[1] for o in out], dtype=np.int32), np.stack([o[2] for o in out]))


# --------------------------------------------------------------------------- cases
def random_grid(shape, density, seed=0, block=True):
    """the grids of the sklearn comparison: default_rng(seed) at `density`, a solid block at [2:8, 3:7, 4:9]"""
    g = np.random.default_rng(seed).random(shape) < density
    if block:
        g[2:8, 3:7, 4:9] = True
    return g


SKLEARN_CASES = (   # shape, density, eps, min_points, voxel_size
    ((12, 13, 17), 0.08, 3.5, 18, None),
    ((16, 16, 16), 0.03, 3.0, 4, None),
    ((9, 20, 33), 0.2, 1.6, 5, (1.3, 0.5, 0.5)),
    ((24, 24, 24), 0.05, 3.5, 18, None),
)

SMALL_SHAPES = ((5, 7, 9), (8, 8, 8), (6, 5, 70), (3, 4, 130), (16, 16, 16))


def small_grid(shape, seed):
    """random positives dense enough for cores at min_points 18 inside eps 3.5, with a solid block where it fits"""
    g = np.random.default_rng(seed).random(shape) < 0.12
    g[1:min(4, shape[0]), 1:4, 2:min(8, shape[2])] = True
    return g


def corner_blobs(shape=(12, 12, 70), size=3):
    """a cube in each of the eight corners and one flush against the middle of every face"""
    g = np.zeros(shape, dtype=bool)
    n = shape
    for c0 in (slice(0, size), slice(n[0] - size, n[0])):
        for c1 in (slice(0, size), slice(n[1] - size, n[1])):
            for c2 in (slice(0, size), slice(n[2] - size, n[2])):
                g[c0, c1, c2] = True
    mid = [slice(m // 2 - 1, m // 2 + 2) for m in n]
    for ax in range(3):
        for face in (slice(0, size), slice(n[ax] - size, n[ax])):
            sl = list(mid)
            sl[ax] = face
            g[tuple(sl)] = True
    return g


def serpentine(n=64, planes=None, lo=0, hi=None, mirror=False):
    """One 1-voxel-wide path through an [n, n, n] grid (n even).  In each plane of `planes` it runs along the rows 0, 2,
    ..., n - 2 over the columns lo..hi, alternating direction, with one voxel in the row between at the turning end; an
    even number of rows, so it enters and leaves every plane at the same end (lo, or hi with `mirror`), where a column
    of voxels through the planes between joins it to the next plane of the list.  Returns (grid, number of voxels by
    the construction).  Under 6-adjacency (eps 1.0) it is one chain."""
    hi = n - 1 if hi is None else hi
    g = np.zeros((n, n, n), dtype=bool)
    planes = list(range(0, n, 2)) if planes is None else list(planes)
    rows = list(range(0, n, 2))
    start = hi if mirror else lo
    count = 0
    up = True             # rows walked in ascending order in this plane
    for k, p in enumerate(planes):
        order = rows if up else rows[::-1]
        at = start
        for j, r in enumerate(order):
            g[p, r, lo:hi + 1] = True
            count += hi - lo + 1
            at = lo + hi - at
            if j + 1 < len(order):
                g[p, (r + order[j + 1]) // 2, at] = True
                count += 1
        assert at == start
        if k + 1 < len(planes):
            for q in range(p + 1, planes[k + 1]):
                g[q, order[-1], start] = True
                count += 1
        up = not up
    return g, count


def two_serpentines(n=64):
    """Two interleaved paths that never touch: A in the planes 0, 4, 8, ... over the columns 0..n-3 with its plane
    changes at column 0, B in the planes 2, 6, 10, ... over the columns 2..n-1 with its plane changes at column n-1.
    Returns (grid, count of A, count of B); A holds voxel (0, 0, 0), so it is cluster 0."""
    a, na = serpentine(n, range(0, n, 4), 0, n - 3)
    b, nb = serpentine(n, range(2, n, 4), 2, n - 1, mirror=True)
    return a, b, na, nb


def isolated_voxels(n=64, step=8, count=100):
    """`count` single voxels `step` apart, in memory order"""
    g = np.zeros((n, n, n), dtype=bool)
    per = n // step
    k = np.arange(count)
    g[(k // (per * per)) * step, ((k // per) % per) * step, (k % per) * step] = True
    return g
