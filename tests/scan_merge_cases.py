"""Scan merge (K19): the numpy oracle -- the three combining rules of include/scenenet_hip.h written out literally, members
from crops_cases.region_mask, bins from binning_cases.expected_flat -- and the inputs its host and GPU tests share.  Every
comparison is exact.  No test lives here."""
import functools

import numpy as np

from oracle import voxel_oracle as vo
from scene_net_amd.crops import lattice_boxes

import binning_cases as bc
import crops_cases as cc

MAX, MEAN, INTERIOR = 0, 1, 2
RULES = (MAX, MEAN, INTERIOR)
DIMS = [(4, 6, 5), (8, 8, 8)]        # (nx, ny, nz): the non-cubic grid catches a swapped axis
CAPACITY = (8, 8, 8)                 # size mode: the table every tile's own dims are padded to
VOXEL_SIZE = (7.0, 7.0, 7.0)
LO, HI = (100.0, 200.0), (170.0, 265.0)
Z_TOP = 80.0                         # taller than a tile is wide: the cube of a tile's lower part ends below its upper points
DISC = (160.0, 230.0, 7.0, 0.0)      # over an inner lattice corner: cover 3 on the seams, 5 on the corner
SEAM_N = (1, 63, 64, 65, 1023, 1024, 1025, 2 * 1024 + 17)
SEAM_K = (1, 3, 64, 65, 130)


# ---- the oracle ----------------------------------------------------------------------------------------------------------
def lesser(a, b):
    """a < b ? a : b, literally"""
    with np.errstate(all="ignore"):
        return np.where(a < b, a, b)


def depth(pts, row, kind):
    """How deep every point lies inside the region, in the header's operations (numpy rounds each once)."""
    x, y = pts[:, 0], pts[:, 1]
    with np.errstate(all="ignore"):
        if kind == cc.DISC:
            dx, dy = x - row[0], y - row[1]
            return np.sqrt(row[2] * row[2]) - np.sqrt(dx * dx + dy * dy)
        return lesser(lesser(x - row[0], row[2] - x), lesser(y - row[1], row[3] - y))


def covering(desc, dims, pts, regions, kinds, tile_of, B, own=None):
    """[(k, t, covered [n] bool, flat [n])] for every region with a tile, in region order"""
    K = regions.shape[0]
    kinds = np.zeros(K, dtype=np.int32) if kinds is None else kinds
    tile_of = np.arange(K) if tile_of is None else tile_of
    out = []
    for k in range(K):
        t = int(tile_of[k])
        if not 0 <= t < B:
            continue
        f = bc.expected_flat(desc[t], dims, pts, None if own is None else own[t])
        out.append((k, t, cc.region_mask(pts, regions[k], int(kinds[k])) & (f >= 0), f))
    return out


def merge_oracle(grid, desc, dims, pts, regions, kinds, tile_of, rule, fill, own=None):
    """(out [C, n] of grid's dtype, cover [n] int32).  grid [B, C, nz, nx, ny]."""
    B, C = grid.shape[:2]
    n = pts.shape[0]
    g = grid.reshape(B, C, -1)
    kinds_ = np.zeros(regions.shape[0], dtype=np.int32) if kinds is None else kinds
    cover = np.zeros(n, dtype=np.int32)
    acc = np.zeros((C, n), dtype=grid.dtype)
    total = np.zeros((C, n), dtype=np.float64)
    best = np.zeros(n, dtype=np.float64)
    for k, t, cov, f in covering(desc, dims, pts, regions, kinds, tile_of, B, own):
        v = g[t][:, np.maximum(f, 0)]
        first = cov & (cover == 0)
        later = cov & (cover > 0)
        with np.errstate(all="ignore"):
            if rule == MAX:
                take = first | (later & ((v > acc) | np.isnan(v)))       # [C, n]
            elif rule == MEAN:
                total = np.where(first, v.astype(np.float64), np.where(later, total + v.astype(np.float64), total))
                take = np.zeros((C, n), dtype=bool)
            else:
                d = depth(pts, regions[k], int(kinds_[k]))
                take1 = first | (later & (d > best))
                best = np.where(take1, d, best)
                take = np.broadcast_to(take1, (C, n))
        acc = np.where(take, v, acc)
        cover = cover + cov
    if rule == MEAN:
        with np.errstate(all="ignore"):
            acc = (total / cover.astype(np.float64)).astype(grid.dtype)
    return np.where(cover > 0, acc, np.asarray(fill, dtype=grid.dtype)).astype(grid.dtype), cover.astype(np.int32)


def max_by_scatter(grid, desc, dims, pts, regions, kinds, tile_of, fill, own=None):
    """MAX in an independent formulation: np.maximum.at over (point, value) pairs, -inf start, `fill` where nothing landed
    (merge_to_scan's own shape).  NaN-free inputs only."""
    B, C = grid.shape[:2]
    g = grid.reshape(B, C, -1)
    out = np.full((C, pts.shape[0]), -np.inf, dtype=grid.dtype)
    seen = np.zeros(pts.shape[0], dtype=bool)
    for k, t, cov, f in covering(desc, dims, pts, regions, kinds, tile_of, B, own):
        idx = np.flatnonzero(cov)
        for c in range(C):
            np.maximum.at(out[c], idx, g[t, c, f[idx]])
        seen[idx] = True
    out[:, ~seen] = fill
    return out


def same_bits(a, b):
    """equal bit for bit, a NaN's payload aside"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    view = np.int32 if a.dtype == np.float32 else np.int64
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(view)[~na], b.view(view)[~nb]))


# ---- the inputs ----------------------------------------------------------------------------------------------------------
TIES = np.array([[130.0, 215.0, 3.0],      # 2.5 deep in x in regions 0 and 3
                 [115.0, 230.0, 4.0],      # 2.5 deep in y in regions 0 and 1
                 [130.0, 230.0, 5.0]])     # the corner of regions 0, 1, 3, 4: 2.5 deep in all four
TIE_WINNER = 0


@functools.lru_cache(maxsize=None)
def main_scan():
    """(pts [n,3], regions [10,4], kinds [10], ties: the rows of TIES in pts).  5000 points uniform over the rectangle, 40
    outside it, 30 with a NaN x and the three tie points, shuffled."""
    rng = np.random.default_rng(190)
    inside = np.column_stack([rng.uniform(LO[0], HI[0], 5000), rng.uniform(LO[1], HI[1], 5000), rng.uniform(0.0, Z_TOP, 5000)])
    outside = np.column_stack([rng.uniform(300.0, 400.0, 40), rng.uniform(LO[1], HI[1], 40), rng.uniform(0.0, Z_TOP, 40)])
    nanx = np.column_stack([np.full(30, np.nan), rng.uniform(LO[1], HI[1], 30), rng.uniform(0.0, Z_TOP, 30)])
    pts = np.concatenate([inside, outside, nanx, TIES])
    order = rng.permutation(len(pts))
    pts = np.ascontiguousarray(pts[order])
    ties = np.array([int(np.flatnonzero(order == len(pts) - 3 + j)[0]) for j in range(3)])
    regions = np.concatenate([lattice_boxes(LO, HI, 30.0, 2.5), np.array([DISC])])
    kinds = np.array([cc.BOX] * 9 + [cc.DISC], dtype=np.int32)
    return pts, regions, kinds, ties


def desc_row(points, dims, sizes=None):
    """(descriptor row padded with +inf to dims, the tile's own dims) of the grid voxelgrid_compute builds from `points`"""
    g = vo.voxelgrid_compute(points, n_xyz=dims if sizes is None else None, sizes=sizes)
    lo, hi, own = g["xyzmin"], g["xyzmax"], tuple(int(v) for v in g["x_y_z"])
    assert all(own[a] <= dims[a] for a in range(3)), (own, dims)
    edges = []
    for a in range(3):
        e = np.full(dims[a] + 1, np.inf)
        e[:own[a] + 1] = vo.linspace_edges(lo[a], hi[a], own[a])
        edges.append(e)
    return np.concatenate([lo, hi] + edges), own


@functools.lru_cache(maxsize=None)
def main_desc(dims, kind="own"):
    """(desc [10, len], own dims [10,3] | None) for the main case's regions.  "own": each tile's grid is built from all its
    members; "foreign": from the lowest 60 % of them in z, so the others bin above the last z edge; "sized": size mode on
    that lower part, padded to `dims`, so the others fall into padding cells."""
    pts, regions, kinds, _ = main_scan()
    rows, owns = [], []
    for k in range(regions.shape[0]):
        m = pts[cc.region_mask(pts, regions[k], int(kinds[k]))]
        if kind != "own":
            m = m[np.argsort(m[:, 2], kind="stable")[:int(0.6 * len(m))]]
        row, own = desc_row(m, dims, VOXEL_SIZE if kind == "sized" else None)
        rows.append(row)
        owns.append(own)
    return np.array(rows), (np.array(owns, dtype=np.int64) if kind == "sized" else None)


def random_grid(B, C, dims, dtype, seed, nans=0):
    """[B, C, nz, nx, ny] of distinct random values; with `nans`, that many cells of every tile and channel are NaN"""
    nx, ny, nz = dims
    rng = np.random.default_rng(seed)
    g = rng.standard_normal((B, C, nz, nx, ny)).astype(dtype)
    if nans:
        flat = g.reshape(B, C, -1)
        for b in range(B):
            for c in range(C):
                flat[b, c, rng.choice(flat.shape[2], nans, replace=False)] = np.nan
    return g


def repeated_regions(K, seed=7):
    """idx [K]: the main case's regions repeated and shuffled to K rows (region k of the result is main region idx[k], and
    reads its tile)"""
    rng = np.random.default_rng(seed + K)
    return rng.permutation(np.resize(rng.permutation(10), K)).astype(np.int32)


def check_inputs():
    """The main case holds what it is there for: each cover value 0, 1, 2, 3 and >= 4 on at least 20 points, and members
    that bin outside a foreign / sized table.  A check of the inputs, not of the code under test."""
    pts, regions, kinds, ties = main_scan()
    desc, _ = main_desc(DIMS[1])
    grid = np.zeros((10, 1) + (8, 8, 8), dtype=np.float32)
    _, cover = merge_oracle(grid, desc, DIMS[1], pts, regions, kinds, None, MAX, 0.0)
    counts = [int((cover == v).sum()) for v in range(4)] + [int((cover >= 4).sum())]
    assert min(counts) >= 20, counts
    assert cover[ties].tolist() == [2, 2, 4]
    for kind in ("foreign", "sized"):
        d, own = main_desc(CAPACITY if kind == "sized" else DIMS[0], kind)
        dims = CAPACITY if kind == "sized" else DIMS[0]
        _, cov = merge_oracle(np.zeros((10, 1, dims[2], dims[0], dims[1]), dtype=np.float32), d, dims, pts, regions, kinds,
                              None, MAX, 0.0, own)
        inside = np.isfinite(pts[:, 0]) & (pts[:, 0] < 200.0)
        assert 500 < int((cov[inside] < cover[inside]).sum()) and int((cov[inside] > 0).sum()) > 1000, kind
        if kind == "sized":
            assert (own < np.array(CAPACITY)).all(), own      # every axis has padding cells
    return counts
