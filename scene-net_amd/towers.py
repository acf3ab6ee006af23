"""Tower proposals on the device: DBSCAN over the voxels of a thresholded prediction (sn_tower_proposals, csrc/towers.hip).

The reference's end product is tower instances: it thresholds the prediction (prob_to_label, utils/voxelization.py:304-323),
turns the positive voxels into points (vxg_to_xyz) and runs open3d's DBSCAN on them, one tile at a time on the host
(eda.extract_towers, utils/pcd_processing.py:577-651, called with eps=3.5, min_points=18 from extract_towers,
compute_euc_dists and get_tower_proposals, utils/observer_utils.py:397-473, 556-).  Here a whole batch is clustered on
the device in six launches, with nothing copied and nothing synchronised:

    props = sna.tower_proposals(pred, tau=0.65)             # labels, n_towers, stats on the device
    towers, centroids = props.towers(b)                     # the reference's return shape for tile b (synchronises)
    towers, centroids = sna.filter_towers(towers, centroids, threshold, center=props.grid_center())

Definition (normative, include/scenenet_hip.h): a voxel is positive if `grid >= tau` in the grid's dtype (NaN is not;
uint8 / bool grids: non-zero); the stencil holds the offsets with (d0 s0)^2 + (d1 s1)^2 + (d2 s2)^2 <= eps^2 (inclusive,
as sklearn's radius query; open3d's boundary rule could not be checked and is unpinned), the voxel itself included; a core
voxel is positive with at least min_points positives of its tile in its stencil; clusters are the connected components of
the cores, numbered by their smallest core voxel; a border voxel (positive, not core, a core in its stencil) takes the
smallest id among those cores; everything else is -1.  Coordinates are grid indices (i0, i1, i2) -- the project's grids are
[nz, nx, ny], so axis 0 is the height -- unless `voxel_size` gives the grid's spacing per axis.  One stencil serves a call:
tiles with spacings of their own are clustered in index units (the default) or one call each.
There is no CPU path: CPU tensors raise HipLibraryError.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _hip
from ._hip import HipLibraryError

STAT_NAMES = ("n_voxels", "n_core", "sum_i0", "sum_i1", "sum_i2", "min_i0", "min_i1", "min_i2", "max_i0", "max_i1",
              "max_i2", "first_core_index")


class TowerProposals:
    """What one sn_tower_proposals call leaves on the device.  Only towers() synchronises; centroids(), boxes() and
    to_world() are device arithmetic on the statistics (no copy in either direction when origin / voxel_size are numbers
    or device tensors), and grid_center() reads no tensor at all.
      labels   [B, n0, n1, n2] int32: the cluster id of every voxel, -1 for noise and for voxels that are not positive
      n_towers [B] int32: the number of clusters, also beyond max_towers
      stats    [B, max_towers, 12] int64 (STAT_NAMES): rows of the ids below max_towers, zero rows for absent clusters
      grids    the VoxelGrids the prediction came from, where ScenePipeline.tower_proposals was given them (else None)"""

    def __init__(self, labels: torch.Tensor, n_towers: torch.Tensor, stats: torch.Tensor, max_towers: int, grids=None):
        self.labels, self.n_towers, self.stats, self.max_towers = labels, n_towers, stats, int(max_towers)
        self.grids = grids

    def _present(self) -> torch.Tensor:
        return self.stats[..., 0] > 0

    def centroids(self) -> torch.Tensor:
        """[B, max_towers, 3] fp64: mean index of each cluster's voxels (sum / count from the integer sums), NaN rows for
        absent clusters."""
        n = self.stats[..., 0:1].to(torch.float64)
        c = self.stats[..., 2:5].to(torch.float64) / n
        return torch.where(self._present()[..., None], c, torch.full_like(c, float("nan")))

    def boxes(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """(lo, hi), each [B, max_towers, 3] fp64: the smallest and largest index of each cluster per axis, NaN rows for
        absent clusters."""
        keep = self._present()[..., None]
        lo, hi = self.stats[..., 5:8].to(torch.float64), self.stats[..., 8:11].to(torch.float64)
        nan = torch.full_like(lo, float("nan"))
        return torch.where(keep, lo, nan), torch.where(keep, hi, nan)

    def to_world(self, origin, voxel_size, index: Optional[torch.Tensor] = None) -> torch.Tensor:
        """origin + index * voxel_size in fp64, the product formed and then added (two roundings, as sn_grid_to_points
        documents).  index: [B, K, 3] in grid-axis order (default: centroids()); origin / voxel_size, in the same axis
        order: 3 numbers (they enter as scalars of the device arithmetic: nothing is copied) or a [3] / per-tile [B, 3]
        tensor on the index's device -- columns of a VoxelGrids.desc can feed it.  A CPU tensor raises."""
        idx = self.centroids() if index is None else index.to(torch.float64)
        B = idx.shape[0]

        def columns(v, name):
            if isinstance(v, torch.Tensor):
                if v.device != idx.device:
                    raise HipLibraryError(f"to_world: {name} must live on {idx.device} (got {v.device}), or be 3 numbers")
                if v.shape not in (torch.Size([3]), torch.Size([B, 3])):
                    raise ValueError(f"{name} must be [3] or [{B}, 3] (got {tuple(v.shape)})")
                t = v.to(torch.float64).reshape(-1, 1, 3)
                return [t[..., k] for k in range(3)]
            vals = [float(x) for x in v]
            if len(vals) != 3:
                raise ValueError(f"{name} must have 3 entries, one per grid axis")
            return vals
        o, s = columns(origin, "origin"), columns(voxel_size, "voxel_size")
        return torch.stack([idx[..., k] * s[k] + o[k] for k in range(3)], dim=-1)

    def grid_center(self) -> np.ndarray:
        """The mean index of all voxels of a tile, (n - 1) / 2 per axis: what filter_towers takes as the grid's centre."""
        return (np.array(self.labels.shape[-3:], dtype=np.float64) - 1.0) / 2.0

    def towers(self, b: int = 0) -> Tuple[List[np.ndarray], np.ndarray]:
        """The reference's return shape for tile b: (list of [n, 3] fp64 arrays of voxel indices, one per cluster in id
        order, voxels in memory order; centroids [K, 3] fp64), all K clusters also beyond max_towers; ([], []) when there
        are none.  Synchronises (copies the tile's labels to the host)."""
        lab = self.labels[b].cpu().numpy()
        idx = np.argwhere(lab >= 0)
        if idx.shape[0] == 0:
            return [], []
        ids = lab[lab >= 0]
        order = np.argsort(ids, kind="stable")
        idx, ids = idx[order].astype(np.float64), ids[order]
        cuts = np.flatnonzero(np.diff(ids)) + 1
        towers = np.split(idx, cuts)
        return towers, np.stack([t.mean(axis=0) for t in towers])


def tower_proposals(grid: torch.Tensor, tau: Optional[float] = None, eps: float = 3.5, min_points: int = 18,
                    voxel_size: Optional[Sequence[float]] = None, max_towers: int = 64) -> TowerProposals:
    """DBSCAN(eps, min_points) over the voxels of `grid` >= tau, per tile (module docstring).  grid: [B,1,n0,n1,n2],
    [B,n0,n1,n2] or [n0,n1,n2]; float32, bfloat16 or float64 with tau in (0, 1), or uint8 / bool (non-zero is positive, tau
    not needed).  voxel_size: the grid's spacing per grid axis (default 1, 1, 1: index units).  Six launches on the current
    stream, no synchronisation: capturable (outputs and scratch come from torch's allocator)."""
    if not isinstance(grid, torch.Tensor) or not grid.is_cuda:
        raise HipLibraryError("tower_proposals: grid must live on a HIP device; there is no CPU path")
    if grid.dim() == 5 and grid.shape[1] == 1:
        g = grid[:, 0]
    elif grid.dim() == 4:
        g = grid
    elif grid.dim() == 3:
        g = grid[None]
    else:
        raise ValueError(f"grid must be [B,1,n0,n1,n2], [B,n0,n1,n2] or [n0,n1,n2] (got {tuple(grid.shape)})")
    is_float = g.dtype in (torch.float32, torch.bfloat16, torch.float64)
    if is_float and tau is None:
        raise ValueError("tau is needed for a float grid")
    g = g.contiguous()
    B, n0, n1, n2 = (int(v) for v in g.shape)
    max_towers = int(max_towers)
    if max_towers < 1:
        raise ValueError("max_towers must be at least 1")
    dev = g.device
    ws = torch.empty(_hip.towers_ws_bytes(B, n0, n1, n2) // 8, dtype=torch.int64, device=dev)
    labels = torch.empty((B, n0, n1, n2), dtype=torch.int32, device=dev)
    n_towers = torch.empty((B,), dtype=torch.int32, device=dev)
    stats = torch.empty((B, max_towers, _hip.SN_TOWER_NSTAT), dtype=torch.int64, device=dev)
    _hip.tower_proposals(g, 0.5 if tau is None else float(tau), float(eps), int(min_points), max_towers, ws, labels,
                         n_towers, stats, voxel_size=voxel_size)
    return TowerProposals(labels, n_towers, stats, max_towers)


# --------------------------------------------------------------------------- #
# Mirrors of utils/observer_utils.py:476-549 on the small per-cluster table (numpy, on the host).  The reference's code
# assumes xyz columns, the height last; our grids are [nz, nx, ny], so the height axis is an argument here and defaults to
# grid axis 0.
def _planar(height_axis: int) -> List[int]:
    if height_axis not in (0, 1, 2):
        raise ValueError("height_axis must be 0, 1 or 2")
    return [a for a in range(3) if a != height_axis]


def filter_towers(towers: Sequence[np.ndarray], centroids, threshold: float, center, height_axis: int = 0,
                  tower_height: float = 14.0, radius: float = 15.0):
    """observer_utils.py:503-549: keeps a cluster if its height reaches `tower_height` or its larger planar extent stays
    within `threshold` (walls are dropped), and only if its centroid lies within radius - 2 * threshold of `center` in
    the plane (a cluster at the rim of the cut-out is no tower).  towers: list of [n, 3] arrays; centroids [C, 3];
    center: 3 numbers (the reference takes the mean of vxg_to_xyz(vxg): TowerProposals.grid_center() in index units).
    Columns are grid axes; `height_axis` names the height (default 0).  Returns (kept towers, centroids[keep])."""
    plane = _planar(height_axis)
    centroids = np.asarray(centroids, dtype=np.float64).reshape(-1, 3)
    center = np.asarray(center, dtype=np.float64)
    keep = np.zeros(len(towers), dtype=bool)
    for i, t in enumerate(towers):
        t = np.asarray(t)
        t_min, t_max = np.min(t, axis=0), np.max(t, axis=0)
        spread = np.max(t_max[plane] - t_min[plane])
        if t_max[height_axis] - t_min[height_axis] >= tower_height:
            keep[i] = True
        else:
            keep[i] = spread <= threshold
        keep[i] = keep[i] and np.sum((centroids[i][plane] - center[plane]) ** 2) <= (radius - threshold * 2) ** 2
    return [towers[i] for i in range(len(towers)) if keep[i]], centroids[keep]


def aggregate_centroids(centroids, height_axis: int = 0, min_euc: float = 1.5) -> np.ndarray:
    """observer_utils.py:476-500: drops the height, replaces every centroid by the mean of the centroids within `min_euc`
    of it in the plane, and returns the distinct rows (np.unique: sorted) -> [M, 2]; an empty input gives [0, 2]."""
    plane = _planar(height_axis)
    if len(centroids) == 0:
        return np.empty((0, 2))
    c = np.asarray(centroids, dtype=np.float64).reshape(-1, 3)[:, plane]
    merged = [np.mean(c[np.linalg.norm(c - v, axis=1) <= min_euc], axis=0) for v in c]
    return np.unique(np.array(merged), axis=0)
