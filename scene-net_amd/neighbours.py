"""A point's neighbourhood on the device: k nearest neighbours within a radius (sn_knn_points / sn_knn_tile_stats,
csrc/knn.hip), and what rests on them -- point spacing, the k-distance curve, outlier removal, and the reference's
avg_dist_points (utils/pcd_processing.py:477-505), its only question about how far apart the points of a cloud are.

    nb = sna.knn_distances(batch, k=8, radius=1.5)            # PointNeighbours: d2, found, mean_dist, index, stats
    mean, std, n_valid, n_full = sna.point_spacing(batch, k=1, radius=1.5)
    curve = sna.k_distance_curve(xyz, k=300, radius=12.0)      # read eps for cluster_points / tower_proposals from it
    clean = sna.remove_outliers(batch, k=8, radius=1.5, std_ratio=2.0)        # ThinnedPoints, as thin_points returns
    clean = sna.remove_outliers(batch, radius=1.5, min_neighbours=4)          # the radius rule
    spacing = sna.avg_dist_points(xyz, 0.5, 5)                 # the reference's call and its literal value

Definition (normative, include/scenenet_hip.h): a candidate of row p is a row q != p of the same tile with (dx*dx + dy*dy) +
dz*dz <= radius*radius in fp64, each product and sum rounded once, the comparison literal (a NaN or infinite coordinate:
no candidates, nobody's candidate); exclude_zero leaves out d2 == 0.  d2 holds the k smallest ascending (+inf beyond),
found counts ALL candidates, mean_dist is the ascending sum of the square roots over their number (NaN for none), index
the packed row indices by the order (d2, row).  The cell grid only decides the speed.
Outlier removal is THIS project's definition: the population std over the rows with a neighbour, a radius-bounded
neighbourhood, no expanding search.  open3d's and PCL's filters are not installed here and their exact conventions (sample
or population std, whether the point counts as its own neighbour) are not pinned.
There is no CPU path: CPU tensors raise HipLibraryError.
"""
from __future__ import annotations

import math
import warnings
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _hip
from ._hip import SN_KNN_MAX_K, SN_KNN_NSTAT, HipLibraryError
from .clusters import _usable_bounds
from .thin import ThinnedPoints, thin_points
from .voxelization import PointBatch

STAT_NAMES = ("n_valid", "n_full", "sum", "sum_sq", "max")
DEFAULT_MAX_CELLS = 1 << 18
_SIDE_MARGIN = 1.0 + 2.0 ** -20


@dataclass
class PointNeighbours:
    """What one knn_distances call leaves on the device, indexed by the packed row (scan order).
      d2        [total, k] f64: the k smallest squared neighbour distances, ascending, +inf beyond the candidates
      found     [total] i32: the number of neighbours within the radius (all of them, not capped at k)
      mean_dist [total] f64 | None: the mean of the min(found, k) distances, NaN for none
      index     [total, k] i64 | None: the neighbours' packed row indices, -1 beyond min(found, k)
      stats     [B, 5] f64 | None (STAT_NAMES): per tile the rows with a neighbour, the rows with k of them, sum, sum of
                squares and max of mean_dist over the former; n_full / n_valid far below 1 says the radius is too small
      offsets   [B+1] i64, radius, k: the call's own"""
    d2: torch.Tensor
    found: torch.Tensor
    mean_dist: Optional[torch.Tensor]
    index: Optional[torch.Tensor]
    stats: Optional[torch.Tensor]
    offsets: torch.Tensor
    radius: float
    k: int

    def distances(self) -> torch.Tensor:
        """[total, k] f64: sqrt(d2), +inf beyond the candidates"""
        return torch.sqrt(self.d2)


def _as_batch(batch_or_xyz) -> Tuple[torch.Tensor, torch.Tensor, Optional[PointBatch]]:
    if isinstance(batch_or_xyz, PointBatch):
        pb = batch_or_xyz
        if not pb.pts.is_cuda:
            raise HipLibraryError("the batch must live on a HIP device; there is no CPU path")
        return pb.pts.to(torch.float64).contiguous(), pb.offsets.to(torch.int64).contiguous(), pb
    t = batch_or_xyz
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise HipLibraryError("xyz must live on a HIP device; there is no CPU path")
    if t.dim() != 2 or t.shape[1] != 3:
        raise ValueError(f"xyz must be [n, 3] (got {tuple(t.shape)})")
    pts = t.to(torch.float64).contiguous()
    return pts, torch.tensor([0, int(pts.shape[0])], dtype=torch.int64, device=pts.device), None


def _grid(extent: Sequence[float], radius: float, B: int, max_cells: int):
    """(dims, mult) of the grid every tile gets: sn_dbscan_cell_grid over the extent with the tile's share of the cells"""
    per_tile = max(1, min(int(max_cells), 1 << 22) // max(B, 1))
    dims, side = _hip.dbscan_cell_grid([0.0, 0.0, 0.0] + [float(v) for v in extent], float(radius), per_tile)
    mult = side / (float(radius) * _SIDE_MARGIN)
    return dims, int(max(1, min(round(mult), 2 ** 62))) if math.isfinite(mult) else 2 ** 62


def _tile_boxes(pts: torch.Tensor, offsets: torch.Tensor):
    """The tiles' boxes from sn_voxel_bbox, an axis without finite coordinates [0, 0]: ONE read to the host"""
    return [_usable_bounds(b) for b in _hip.voxel_bbox(pts, offsets).cpu().tolist()]


def _tile_grid(pts: torch.Tensor, offsets: torch.Tensor, radius: float, lo, extent, max_cells: int, box=None):
    """(lo [3 B] f64 on the device, dims, mult) of the tiles' search grids.  lo / extent None: from the tiles' boxes (`box`,
    or ONE read to the host); both given, nothing is read."""
    B = int(offsets.numel()) - 1
    if lo is None or extent is None:
        box = _tile_boxes(pts, offsets) if box is None else box
        if extent is None:
            extent = [max(b[3 + a] - b[a] for b in box) for a in range(3)]
        if lo is None:
            lo = torch.tensor([b[:3] for b in box], dtype=torch.float64, device=pts.device)
    if not isinstance(lo, torch.Tensor) or not lo.is_cuda:
        raise HipLibraryError("lo must live on a HIP device; there is no CPU path")
    lo = lo.to(torch.float64).reshape(-1).contiguous()
    if lo.numel() != 3 * B:
        raise ValueError(f"lo must be [B, 3] = [{B}, 3]")
    return (lo, *_grid(extent, radius, B, max_cells))


def knn_distances(batch_or_xyz: Union[PointBatch, torch.Tensor], k: int, radius: Optional[float] = None,
                  exclude_zero: bool = False, want_index: bool = False, want_mean: bool = True, lo=None, extent=None,
                  max_cells: int = DEFAULT_MAX_CELLS, want_stats: Optional[bool] = None) -> PointNeighbours:
    """The k nearest neighbours within `radius` of every row of a PointBatch (tiles never see each other) or of xyz [n,3]
    on the device (one tile); module docstring.  k in 1 .. 16.
      lo, extent  lo [B,3] (device tensor) and extent (3 host floats): where each tile's search grid starts and how far it
                  reaches.  Both given: no synchronisation, capturable (radius is needed then).  Otherwise the tiles' boxes
                  come from sn_voxel_bbox with ONE read to the host; an axis without finite coordinates gets [0, 0].  The
                  result is exact for any lo and extent -- they only decide the speed.
      radius      None: the largest tile diagonal times (1 + 1e-6), i.e. every other point of the tile is a candidate and
                  every tile is ONE cell: brute force on the device, O(n^2).  For small sets and for avg_dist_points.
      max_cells   the cell budget of the whole batch (at most 2^22)
      want_stats  the tile statistics (default: iff want_mean)"""
    pts, offsets, _ = _as_batch(batch_or_xyz)
    k = int(k)
    if k < 1:
        raise ValueError("k must be at least 1")
    if k > SN_KNN_MAX_K:
        raise ValueError(f"k = {k} is beyond the {SN_KNN_MAX_K} neighbours the kernel keeps in registers")
    want_stats = want_mean if want_stats is None else bool(want_stats)
    if want_stats and not want_mean:
        raise ValueError("the tile statistics are those of mean_dist: want_mean is needed")
    dev, total, B = pts.device, int(pts.shape[0]), int(offsets.numel()) - 1
    if total == 0 or B < 1:
        raise ValueError("knn_distances needs at least one point")
    box = None
    if radius is None:
        box = _tile_boxes(pts, offsets)                             # the one read
        diag = max(math.sqrt(sum((b[3 + a] - b[a]) ** 2 for a in range(3))) for b in box)
        radius = max(diag, 1e-9) * (1.0 + 1e-6)
        extent = [0.0, 0.0, 0.0]                                    # one cell per tile
    lo, dims, mult = _tile_grid(pts, offsets, radius, lo, extent, max_cells, box)
    radius = float(radius)
    ws = torch.empty(_hip.knn_ws_bytes(total, B, dims[0] * dims[1] * dims[2]) // 8, dtype=torch.int64, device=dev)
    d2 = torch.empty((total, k), dtype=torch.float64, device=dev)
    found = torch.empty((total,), dtype=torch.int32, device=dev)
    mean = torch.empty((total,), dtype=torch.float64, device=dev) if want_mean else None
    index = torch.empty((total, k), dtype=torch.int64, device=dev) if want_index else None
    _hip.knn_points(pts, offsets, radius, k, lo, dims, mult, ws, d2, found, mean, index, exclude_zero=exclude_zero)
    stats = None
    if want_stats:
        stats = torch.empty((B, SN_KNN_NSTAT), dtype=torch.float64, device=dev)
        _hip.knn_tile_stats(mean, found, offsets, k, ws, stats)
    return PointNeighbours(d2, found, mean, index, stats, offsets, radius, k)


def _spacing_of(stats: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(mean [B], population std [B]) of mean_dist over the valid rows; NaN for a tile without one"""
    n, s, sq = stats[:, 0], stats[:, 2], stats[:, 3]
    mean = s / n
    var = torch.clamp(sq / n - mean * mean, min=0.0)        # (0 / 0 = NaN stays NaN through clamp)
    return mean, torch.sqrt(var)


def point_spacing(batch, k: int = 1, radius: Optional[float] = None, **grid):
    """(mean [B], std [B], n_valid [B], n_full [B]) on the device: mean and POPULATION std of every row's mean distance to
    its min(found, k) nearest neighbours within `radius`, over the rows that have one; n_valid of them, n_full with k.
    A tile without a valid row gives NaN.  `grid`: lo, extent, max_cells of knn_distances."""
    nb = knn_distances(batch, k, radius, **grid)
    mean, std = _spacing_of(nb.stats)
    return mean, std, nb.stats[:, 0].to(torch.int64), nb.stats[:, 1].to(torch.int64)


def k_distance_curve(xyz, k: int, radius: float, **grid) -> torch.Tensor:
    """The distances to the k-th nearest neighbour of the rows that have k neighbours within `radius`, sorted descending:
    the curve whose knee is DBSCAN's eps for min_points = k (+ 1 where the point itself counts, as in cluster_points).
    A torch.sort on the device, not a kernel.  Synchronises (the result's length is data)."""
    nb = knn_distances(xyz, k, radius, want_mean=False, **grid)
    kth = torch.sqrt(nb.d2[:, k - 1][nb.found >= k])
    return torch.sort(kth, descending=True).values


def remove_outliers(batch, k: int = 8, radius: Optional[float] = None, std_ratio: float = 2.0,
                    min_neighbours: Optional[int] = None, capacity: Optional[int] = None, labels=None,
                    **grid) -> ThinnedPoints:
    """Drops the stray returns of every tile and returns the rest as thin_points does (scan order, labels, src).
      statistical rule (min_neighbours None): a row is kept iff mean_dist <= mean_b + std_ratio * std_b, with mean_b and
        std_b the tile's mean and POPULATION std of mean_dist over its rows with a neighbour; a row with no neighbour
        within `radius` (NaN) is dropped.
      radius rule (min_neighbours given): a row is kept iff found >= min_neighbours (k plays no part in it).
    This is this project's own definition (module docstring): open3d's and PCL's conventions are not pinned.
    Both go through thin_points(u=..., thresholds=[B, 1]) -- the rule there is u <= thr with NaN keeping nothing; the radius
    rule passes u = -found, thr = -min_neighbours.  With `capacity` (and lo / extent in `grid`) nothing is read back: the
    chain is capturable.  batch: a PointBatch, or xyz [n,3] with `labels`."""
    if radius is None:
        raise ValueError("remove_outliers needs a radius: the neighbourhood is bounded by it")
    pts, offsets, pb = _as_batch(batch)
    if pb is None:
        lab = None if labels is None else labels.to(torch.float64).reshape(-1).contiguous()
        pb = PointBatch(pts, lab, offsets, (int(pts.shape[0]),))
    elif labels is not None:
        raise ValueError("labels come with the PointBatch")
    B = int(offsets.numel()) - 1
    if min_neighbours is None:
        nb = knn_distances(pb, k, radius, **grid)
        mean, std = _spacing_of(nb.stats)
        u, thr = nb.mean_dist, (mean + float(std_ratio) * std).reshape(B, 1)
    else:
        nb = knn_distances(pb, 1, radius, want_mean=False, **grid)
        u = -nb.found.to(torch.float64)
        thr = torch.full((B, 1), -float(int(min_neighbours)), dtype=torch.float64, device=pts.device)
    return thin_points(pb, thresholds=thr, u=u, capacity=capacity)


def _running_means(table: np.ndarray, num_dists: int) -> np.ndarray:
    """avgs of avg_dist_points from table [m, num_dists]: each row's num_dists smallest positive distances ascending, +inf
    where it has fewer.  The reference's list after point i holds the positive distances of the points 0..i; its num_dists
    smallest lie among each of those rows' own num_dists smallest, so the merge below is the reference's
    np.sort(dists)[:num_dists] and np.mean, value for value."""
    avgs, dists = [], np.empty(0, dtype=np.float64)
    for row in table:
        dists = np.sort(np.concatenate([dists, row[np.isfinite(row)]]))[:num_dists]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")     # (the mean of no distance yet is NaN, as in the reference)
            avgs.append(np.mean(dists))
    return np.array(avgs, dtype=np.float64)


def avg_dist_points(xyz, accuracy: float, num_dists: int) -> float:
    """pcd_processing.py:477-505 with its literal value: over the first round(len(xyz) * accuracy) points, avgs[i] is the
    mean of the num_dists smallest positive distances from the points 0..i to all points of that view (the reference's
    list is never cleared; a pair appears twice once both ends are in), and the result is np.mean(avgs).
    The device computes every row's num_dists smallest positive distances (knn_distances with radius None -- brute force,
    O(m^2) like the original -- and exclude_zero); the table of m * num_dists doubles is copied down and the running merge
    and the two means run on the HOST with the reference's own numpy sequence: that part is not a kernel.
    A distance here is sqrt((dx*dx + dy*dy) + dz*dz); np.linalg.norm may differ from it in the last place, so the value
    agrees with the reference's within (num_dists + m + 4) * 2^-53 relative, not bit for bit.  num_dists <= 16."""
    num_dists = int(num_dists)
    if num_dists > SN_KNN_MAX_K:
        raise ValueError(f"num_dists = {num_dists} is beyond the limit of {SN_KNN_MAX_K} neighbours the kernel keeps")
    if num_dists < 1:
        raise ValueError("num_dists must be at least 1")
    if isinstance(xyz, np.ndarray):
        xyz = torch.from_numpy(np.ascontiguousarray(xyz[:, :3], dtype=np.float64)).to(
            torch.device("cuda", torch.cuda.current_device()))
    if not isinstance(xyz, torch.Tensor) or not xyz.is_cuda:
        raise HipLibraryError("xyz must live on a HIP device; there is no CPU path")
    view = xyz[:round(int(xyz.shape[0]) * accuracy), :3]
    if view.shape[0] == 0:
        return float("nan")                     # (np.mean of no average)
    nb = knn_distances(view, num_dists, radius=None, exclude_zero=True, want_mean=False)
    return float(np.mean(_running_means(nb.distances().cpu().numpy(), num_dists)))
