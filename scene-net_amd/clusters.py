"""The towers of a labelled scan on the device: point DBSCAN (sn_points_select / sn_dbscan_points, csrc/dbscan.hip).

The reference finds the towers of a scan on the host (utils/pcd_processing.py: select_object :508-522, then extract_towers
:577-651 -- open3d's cluster_dbscan(eps=10, min_points=300) over the tower-labelled points and a pandas group-by) in front
of crop_tower_samples and crop_two_towers_samples (:765-817), which core/datasets/ts40k.py:86-92 build_data_samples
drives.  Here the scan stays in HBM from the labels to the samples:

    found = sna.cluster_points(scan_xyz, eps=10, min_points=300, labels=scan_classes, keep=[15])
    towers = found.towers()                                   # list of [n_k, 3], id order, scan order inside
    samples = sna.crop_tower_samples(scan_xyz, scan_classes)  # the reference's own signature: K10, then one K9 pass

Definition (normative, include/scenenet_hip.h): a point is selected iff its label equals one of `keep` (np.isin: a NaN
label never is; without labels every point is); the selected points keep scan order and their positions 0..m-1 are the
indices.  q is a neighbour of p iff (dx*dx + dy*dy) + dz*dz <= eps*eps in fp64, each product and sum rounded once, p
itself included, the comparison literal (a NaN or infinite coordinate: nobody's neighbour, noise).  A core point has at
least min_points neighbours; clusters are the connected components of the cores, numbered by their smallest core
position; a border point (not core, a core neighbour) takes the smallest id among its core neighbours; the rest is -1.
sklearn's DBSCAN(algorithm='kd_tree') gives the same labels on sets with no pair on the rim; open3d's boundary rule and
its choice for a border that two clusters reach could not be checked and are unpinned, as for tower_proposals.
There is no CPU path: CPU tensors raise HipLibraryError.
"""
from __future__ import annotations

import math
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _hip
from ._hip import SN_CROP_BOX, HipLibraryError
from .voxelization import _device_f64

STAT_NAMES = ("n_points", "n_core", "first_core_index")
DEFAULT_MAX_CELLS = 1 << 18


class PointClusters:
    """What one cluster_points call leaves on the device.
      sel        [capacity] int64 | None: the scan index of every selected position (None: the scan's own rows)
      cluster    [capacity] int32: the cluster id per position, -1 for noise; rows beyond min(n_sel, capacity) are unset
      n_sel      [1] int64: the TRUE number of selected points, also beyond the capacity
      n_clusters [1] int32: the number of clusters, also beyond max_clusters
      stats      [max_clusters, 3] int64 (STAT_NAMES): rows of the ids below max_clusters, zero rows for absent clusters
      status     [1] int32: bit 0 set iff n_sel > capacity (the clustering saw the first `capacity` positions only)
    Only towers(), src() and check() synchronise."""

    def __init__(self, pts: torch.Tensor, sel: Optional[torch.Tensor], cluster: torch.Tensor, n_sel: torch.Tensor,
                 n_clusters: torch.Tensor, stats: torch.Tensor, status: torch.Tensor, max_clusters: int):
        self.pts, self.sel, self.cluster, self.n_sel = pts, sel, cluster, n_sel
        self.n_clusters, self.stats, self.status, self.max_clusters = n_clusters, stats, status, int(max_clusters)

    @property
    def capacity(self) -> int:
        return int(self.cluster.numel())

    def check(self) -> int:
        """Raises if the status is set; returns the number of positions that were clustered.  Synchronises."""
        n_sel, status = int(self.n_sel), int(self.status)
        if status & 1:
            raise HipLibraryError(f"{n_sel} points were selected, beyond the capacity of {self.capacity}: the clustering "
                                  "saw the first positions only")
        return min(n_sel, self.capacity)

    def _groups(self) -> Tuple[torch.Tensor, List[int]]:
        """(scan indices sorted by cluster id, stable; sizes [noise, cluster 0, cluster 1, ...])"""
        m = self.check()
        cl = self.cluster[:m].to(torch.int64)
        order = torch.argsort(cl, stable=True)
        sizes = torch.bincount(cl + 1, minlength=1).cpu().tolist() if m else [0]
        return (order if self.sel is None else self.sel[:m][order]), sizes

    def towers(self) -> List[torch.Tensor]:
        """The reference's return shape: a list of [n_k, 3] tensors, one per cluster in id order, each in scan order
        (all K clusters, also beyond max_clusters); [] when there is none.  Synchronises; raises on a set status."""
        src, sizes = self._groups()
        out, at = [], sizes[0]
        for s in sizes[1:]:
            out.append(self.pts[src[at:at + s]])
            at += s
        return out

    def src(self, k: int) -> torch.Tensor:
        """The scan indices of cluster k, ascending.  Synchronises; raises on a set status."""
        src, sizes = self._groups()
        if not 0 <= k < len(sizes) - 1:
            raise IndexError(f"cluster {k} of {len(sizes) - 1}")
        at = sum(sizes[:k + 1])
        return src[at:at + sizes[k + 1]]


def _keep_tensor(keep, dev) -> torch.Tensor:
    if isinstance(keep, torch.Tensor):
        if not keep.is_cuda:
            raise HipLibraryError("keep must be a sequence of numbers or live on a HIP device")
        return keep.to(torch.float64).reshape(-1).contiguous()
    return torch.tensor([float(v) for v in np.asarray(keep, dtype=np.float64).reshape(-1)], dtype=torch.float64, device=dev)


def _usable_bounds(b: Sequence[float]) -> List[float]:
    """bbox of a selection -> bounds the grid takes: an axis without a finite coordinate gets [0, 0]"""
    b = [float(v) for v in b]
    for a in range(3):
        if not (math.isfinite(b[a]) and math.isfinite(b[3 + a]) and b[a] <= b[3 + a]):
            b[a] = b[3 + a] = 0.0
    return b


def cluster_points(pts: torch.Tensor, eps: float, min_points: int, labels: Optional[torch.Tensor] = None, keep=None,
                   capacity: Optional[int] = None, bounds: Optional[Sequence[float]] = None, max_clusters: int = 64,
                   max_cells: int = DEFAULT_MAX_CELLS) -> PointClusters:
    """DBSCAN(eps, min_points) over the points of pts [n,3] whose label is one of `keep` (all points without labels);
    module docstring.  keep: numbers, or a device tensor (needed inside a capture).
    capacity None or bounds None: select, ONE read of n_sel and the selection's box to the host, exact allocation,
    cluster.  Both given: the two entries run back to back with no synchronisation (capturable); `capacity` positions are
    clustered at most and status tells whether more were selected; `bounds` = (xmin, ymin, zmin, xmax, ymax, zmax) only
    lays out the search grid (at most max_cells cells) -- the result is exact for any bounds."""
    pts = _device_f64(pts, "pts")
    if pts.dim() != 2 or pts.shape[1] != 3:
        raise ValueError(f"pts must be [n, 3] (got {tuple(pts.shape)})")
    if (labels is None) != (keep is None):
        raise ValueError("labels and keep are given together")
    dev, n = pts.device, int(pts.shape[0])
    max_clusters = int(max_clusters)
    if max_clusters < 1:
        raise ValueError("max_clusters must be at least 1")
    if capacity is not None and int(capacity) < 0:
        raise ValueError("capacity must not be negative")
    head = torch.zeros(8, dtype=torch.int64, device=dev)     # n_sel, the box, status: one read serves all
    n_sel, bbox, status = head[0:1], head[1:7].view(torch.float64), head[7:8].view(torch.int32)[0:1]
    n_clusters = torch.zeros(1, dtype=torch.int32, device=dev)
    stats = torch.zeros((max_clusters, _hip.SN_DBSCAN_NSTAT), dtype=torch.int64, device=dev)
    one_read = capacity is None or bounds is None
    rows = (n if capacity is None else int(capacity))
    sel = None
    if n > 0:
        if labels is not None:
            labels = _device_f64(labels, "labels").reshape(-1)
            keep = _keep_tensor(keep, dev)
            sel = torch.empty(rows, dtype=torch.int64, device=dev)
        if labels is not None or bounds is None:
            ws = torch.empty(_hip.points_select_ws_bytes(n) // 8, dtype=torch.int64, device=dev)
            _hip.points_select(pts, labels, keep, ws, sel, n_sel, bbox)
        else:
            n_sel.fill_(n)
    m = rows
    if one_read:
        got = head.cpu()
        told = int(got[0]) if n > 0 else 0
        m = told if capacity is None else min(told, rows)
        if bounds is None:
            bounds = _usable_bounds(got[1:7].view(torch.float64).tolist())
        if capacity is None:
            rows = m
            if sel is not None:
                sel = sel[:m].clone()
    cluster = torch.empty(rows, dtype=torch.int32, device=dev)
    if n > 0 and rows > 0 and m > 0:
        dims, _ = _hip.dbscan_cell_grid(bounds, eps, max_cells)
        ws = torch.empty(_hip.dbscan_ws_bytes(rows, dims[0] * dims[1] * dims[2]) // 8, dtype=torch.int64, device=dev)
        _hip.dbscan_points(pts, sel, n_sel, bounds, float(eps), int(min_points), int(max_cells), max_clusters, ws, cluster,
                           n_clusters, stats, status)
    else:
        status.copy_((n_sel > rows).to(torch.int32))     # (device arithmetic: nothing is read back)
    return PointClusters(pts, sel, cluster, n_sel, n_clusters, stats, status, max_clusters)


# --------------------------------------------------------------------------- #
# Mirrors of utils/pcd_processing.py with the reference's signatures; tensors on the device replace the arrays and the
# open3d point cloud.
def select_object(xyz: torch.Tensor, classes: torch.Tensor, obj_class) -> Tuple[torch.Tensor, torch.Tensor]:
    """pcd_processing.py:508-522: (the points whose class is one of obj_class [m, 3], in scan order; the classes of ALL
    points as float64, the reference's second value).  One read of the count (synchronises)."""
    xyz = _device_f64(xyz, "xyz")
    classes = _device_f64(classes, "classes").reshape(-1)
    n, dev = int(xyz.shape[0]), xyz.device
    if n == 0:
        return xyz, classes
    keep = _keep_tensor(obj_class, dev)
    head = torch.zeros(7, dtype=torch.int64, device=dev)
    sel = torch.empty(n, dtype=torch.int64, device=dev)
    ws = torch.empty(_hip.points_select_ws_bytes(n) // 8, dtype=torch.int64, device=dev)
    _hip.points_select(xyz, classes, keep, ws, sel, head[0:1], head[1:7].view(torch.float64))
    return xyz[sel[:int(head[0])]], classes


def extract_towers(xyz_towers: torch.Tensor, eps: float = 10, min_points: int = 300) -> List[torch.Tensor]:
    """pcd_processing.py:577-651: the points of each cluster of DBSCAN(eps, min_points) over xyz_towers [m, 3] -> list of
    [n_k, 3] tensors in id order (the reference's order is that of np.unique over open3d's colours), [] for none."""
    return cluster_points(xyz_towers, eps, min_points).towers()


def crop_two_towers_samples(xyz: torch.Tensor, classes: torch.Tensor, obj_class=(15,), eps: float = 10,
                            min_points: int = 300) -> List[torch.Tensor]:
    """pcd_processing.py:765-801: every tower is paired with the nearest other tower by mean; the sample [n, 4] (x, y, z,
    class) is the box crop of the pair (crop_two_towers) followed by the height-radius disc crops of the two towers
    (crop_tower_radius with radius 0); a pair whose box crop is empty is skipped; fewer than two towers give [].  The
    towers come from cluster_points, and ONE crop_regions pass cuts every box and disc."""
    from .crops import _tiles, _tower_disc, crop_regions
    xyz = _device_f64(xyz, "xyz")
    towers = cluster_points(xyz, eps, min_points, labels=classes, keep=obj_class).towers()
    K = len(towers)
    if K < 2:
        return []
    means = torch.stack([torch.mean(t, dim=0) for t in towers]).cpu().numpy()
    pair = []
    for i in range(K):
        eucs = np.array([np.linalg.norm(means[i] - means[j]) for j in range(K)])
        idx = int(np.argmin(eucs[eucs > 0]))      # eucs == 0 is the distance with itself
        pair.append(idx + 1 if idx >= i else idx)
    boxes = []
    for i in range(K):
        tt = torch.cat([towers[i], towers[pair[i]]])
        lo, hi = tt.min(dim=0).values, tt.max(dim=0).values
        boxes.append(torch.stack([lo[0], lo[1], hi[0], hi[1]]))
    regions = torch.cat([torch.stack(boxes)] + [_tower_disc(t, 0) for t in towers])
    kinds = torch.zeros(2 * K, dtype=torch.int32, device=xyz.device)
    kinds[:K] = SN_CROP_BOX
    tiles = [torch.cat([p, l[:, None]], dim=1) for p, l in _tiles(crop_regions(xyz, regions, kinds, classes, want_src=False))]
    return [torch.cat([tiles[i], tiles[K + i], tiles[K + pair[i]]]) for i in range(K) if tiles[i].shape[0] > 0]
