"""Tiles cut out of a whole scan on the device: disc and box crops (sn_crop_count / sn_crop_scatter, csrc/crops.hip).

The reference cuts its training and inference tiles on the host (utils/pcd_processing.py: crop_at_locations :820-840,
crop_tower_radius :666-697, crop_two_towers :700-739, crop_tower_samples :805-817, which core/datasets/ts40k.py:31-148
build_data_samples drives): `a[mask]` over the whole cloud, once per centre.  Here K regions are cut in one pass over a
scan that stays in HBM, and what comes back is a CSR batch K1 takes as it is:

    regions, kinds = sna.lattice_regions(lo_xy, hi_xy, tile=30.0, overlap=5.0)
    crops = sna.crop_regions(scan_xyz, regions, kinds)              # ScanCrops: pts, labels, src, offsets
    batch, kept = crops.point_batch()                               # empty tiles dropped
    out, per_point = sna.ScenePipeline(model, per_point=True)(batch)
    scan_pred = sna.merge_to_scan(per_point[0], crops.src_rows(), n=scan_xyz.shape[0])

Definition (normative, include/scenenet_hip.h): a disc row (cx, cy, r, unused) holds a point iff
(x-cx)*(x-cx) + (y-cy)*(y-cy) <= r*r in fp64, each product and the sum rounded once -- numpy's
np.sum(np.power(xyz[:, :2] - c[:2], 2), axis=1) <= radius*radius bit for bit; a box row (xmin, ymin, xmax, ymax) iff
xmin <= x <= xmax and ymin <= y <= ymax, inclusive.  z takes no part.  Comparisons are literal: NaN is in no region, a
negative r behaves as |r|, a box with min > max is empty, a kinds value other than 0 / 1 makes the region empty.  Tile k
holds region k's members in scan order; values travel as 64-bit patterns.
There is no CPU path: CPU tensors raise HipLibraryError.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _hip
from ._hip import SN_CROP_BOX, HipLibraryError
from .voxelization import PointBatch, _device_f64


@dataclass
class ScanCrops:
    """What one crop_regions call leaves on the device: a CSR batch of K tiles.
      pts     [total | capacity, 3] f64, labels [..] f64 | None, src [..] int64 | None (each row's index in the scan)
      offsets [K+1] int64: the TRUE sizes, also where a given capacity was too small
      regions [K,4] f64, kinds [K] int32 | None: what was asked for"""
    pts: torch.Tensor
    labels: Optional[torch.Tensor]
    src: Optional[torch.Tensor]
    offsets: torch.Tensor
    regions: torch.Tensor
    kinds: Optional[torch.Tensor]

    @property
    def K(self) -> int:
        return int(self.offsets.numel()) - 1

    def sizes(self) -> Tuple[int, ...]:
        """Points per tile (copies offsets to the host: synchronises)."""
        off = self.offsets.cpu().numpy()
        return tuple(int(v) for v in np.diff(off))

    def tile(self, k: int):
        """(pts [n_k,3], labels [n_k] | None, src [n_k] | None) of tile k: views (reads two offsets: synchronises)."""
        lo, hi = (int(v) for v in self.offsets[k:k + 2].cpu())
        if hi > self.pts.shape[0]:
            raise HipLibraryError(f"tile {k} ends at row {hi}, beyond the capacity of {self.pts.shape[0]} rows")
        return (self.pts[lo:hi], None if self.labels is None else self.labels[lo:hi],
                None if self.src is None else self.src[lo:hi])

    def point_batch(self, drop_empty: bool = True) -> Tuple[PointBatch, List[int]]:
        """(PointBatch, indices of the regions it holds).  An empty tile cannot be voxelised (PointBatch.from_tiles raises
        for one, as the reference's pyntcloud does): with drop_empty the empty tiles leave the CSR table -- their rows are
        none, so pts / labels are shared, not copied -- otherwise one raises ValueError.  Synchronises (sizes)."""
        sizes = self.sizes()
        total = sum(sizes)
        if total > self.pts.shape[0]:
            raise HipLibraryError(f"the crops hold {total} rows, beyond the capacity of {self.pts.shape[0]}")
        kept = [k for k, s in enumerate(sizes) if s > 0]
        if len(kept) != len(sizes) and not drop_empty:
            raise ValueError("zero-size array to reduction operation minimum which has no identity (empty tile)")
        if not kept:
            raise ValueError("every crop is empty: there is nothing to voxelise")
        if len(kept) == len(sizes):
            offsets = self.offsets
        else:
            offsets = torch.cat([self.offsets[:1], self.offsets[1:][torch.tensor(kept, device=self.offsets.device)]])
        return (PointBatch(self.pts[:total], None if self.labels is None else self.labels[:total], offsets,
                           tuple(sizes[k] for k in kept)), kept)

    def src_rows(self) -> torch.Tensor:
        """src of the rows the crops hold, offsets[K] of them (reads it: synchronises) -- the rows of point_batch(), which
        drops tiles, never rows."""
        if self.src is None:
            raise HipLibraryError("the crops were made with want_src=False")
        return self.src[:int(self.offsets[-1])]


def crop_regions(pts: torch.Tensor, regions: torch.Tensor, kinds: Optional[torch.Tensor] = None,
                 labels: Optional[torch.Tensor] = None, capacity: Optional[int] = None, want_src: bool = True) -> ScanCrops:
    """Cuts the K regions out of the scan pts [n,3] (labels [n] optional), all tensors on the device (module docstring).
    capacity None: count, ONE read of offsets[K] to the host, exact allocation, scatter.  capacity int: count and scatter
    back to back with no synchronisation (capturable); pts / labels / src have `capacity` rows, rows beyond offsets[K] are
    uninitialised, and whether the crops fit is the caller's to check from offsets[K]."""
    pts = _device_f64(pts, "pts")
    regions = _device_f64(regions, "regions")
    if labels is not None:
        labels = _device_f64(labels, "labels").reshape(-1)
    if kinds is not None:
        if not isinstance(kinds, torch.Tensor) or not kinds.is_cuda:
            raise HipLibraryError("kinds must live on a HIP device; there is no CPU path")
        kinds = kinds.to(torch.int32).contiguous()
    if pts.dim() != 2 or pts.shape[1] != 3:
        raise ValueError(f"pts must be [n, 3] (got {tuple(pts.shape)})")
    if regions.dim() != 2 or regions.shape[1] != 4:
        raise ValueError(f"regions must be [K, 4] (got {tuple(regions.shape)})")
    n, K = int(pts.shape[0]), int(regions.shape[0])
    if n == 0 or K == 0:
        raise ValueError("crop_regions needs at least one point and one region")
    dev = pts.device
    ws = torch.empty(_hip.crops_ws_bytes(n, K) // 8, dtype=torch.int64, device=dev)
    offsets = torch.empty(K + 1, dtype=torch.int64, device=dev)
    _hip.crop_count(pts, regions, kinds, ws, offsets)
    rows = int(offsets[-1]) if capacity is None else int(capacity)
    if rows < 0:
        raise ValueError("capacity must not be negative")
    out_pts = torch.empty((rows, 3), dtype=torch.float64, device=dev)
    out_labels = torch.empty((rows,), dtype=torch.float64, device=dev) if labels is not None else None
    out_src = torch.empty((rows,), dtype=torch.int64, device=dev) if want_src else None
    if rows > 0:   # (an empty buffer has no address to hand over, and nothing could be written to it)
        _hip.crop_scatter(pts, labels, regions, kinds, ws, offsets, out_pts, out_labels, out_src)
    return ScanCrops(out_pts, out_labels, out_src, offsets, regions, kinds)


# --------------------------------------------------------------------------- #
# Mirrors of utils/pcd_processing.py with the reference's signatures and return conventions; tensors on the device replace
# the arrays.  Radii and centres that the reference derives from the data (`radius == 0`, a tower's mean) are computed on
# the device and written into the region rows there: nothing is read back before the crop.
def _discs(centres_xy: torch.Tensor, radius) -> torch.Tensor:
    """rows (cx, cy, r, 0) from centres [K,2] and a radius (a number or a 0-dim device tensor)"""
    K = centres_xy.shape[0]
    rows = torch.zeros((K, 4), dtype=torch.float64, device=centres_xy.device)
    rows[:, :2] = centres_xy
    rows[:, 2] = radius
    return rows


def _tiles(crops: ScanCrops) -> List[Tuple[torch.Tensor, Optional[torch.Tensor]]]:
    off = crops.offsets.cpu().tolist()
    return [(crops.pts[a:b], None if crops.labels is None else crops.labels[a:b]) for a, b in zip(off, off[1:])]


def crop_at_locations(xyz: torch.Tensor, coords: torch.Tensor, radius: float = 0, classes: Optional[torch.Tensor] = None
                      ) -> List[torch.Tensor]:
    """pcd_processing.py:820-840: one disc per row of coords [K, 3] (the last column is not read) -> list of [n_k, 3]
    tensors, [n_k, 4] with the class as the last column when classes is given.  radius == 0: the scan's z extent,
    computed on the device and placed into the region rows without a synchronisation."""
    xyz = _device_f64(xyz, "xyz")
    coords = _device_f64(coords, "coords")
    coords = coords.reshape(-1, coords.shape[-1])
    r = (xyz[:, 2].max() - xyz[:, 2].min()) if radius == 0 else float(radius)
    crops = crop_regions(xyz, _discs(coords[:, :2], r), None, classes, want_src=False)
    return [p if l is None else torch.cat([p, l[:, None]], dim=1) for p, l in _tiles(crops)]


def _tower_disc(xyz_tower: torch.Tensor, radius) -> torch.Tensor:
    t = _device_f64(xyz_tower, "xyz_tower")
    r = (t[:, 2].max() - t[:, 2].min()) if radius == 0 else float(radius)
    return _discs(torch.mean(t, dim=0)[None, :2], r)


def crop_tower_radius(xyz: torch.Tensor, classes: torch.Tensor, xyz_tower: torch.Tensor, radius: float = 0
                      ) -> Tuple[torch.Tensor, torch.Tensor]:
    """pcd_processing.py:666-697: the points within `radius` (in the plane) of the tower's mean -> (pts [n,3], classes [n]
    int64).  radius == 0: the tower's height.  The mean is torch.mean on the device: its summation order is not numpy's,
    so a centre may differ by an ulp from the reference's (and a point on the rim with it)."""
    xyz = _device_f64(xyz, "xyz")
    crops = crop_regions(xyz, _tower_disc(xyz_tower, radius), None, classes, want_src=False)
    return crops.pts, crops.labels.to(torch.int64)


def crop_two_towers(xyz: torch.Tensor, classes: torch.Tensor, xyz_tower1: torch.Tensor, xyz_tower2: torch.Tensor
                    ) -> Tuple[torch.Tensor, torch.Tensor]:
    """pcd_processing.py:700-739: the points inside the xy bounding box of both towers, inclusive -> (pts, classes int64)."""
    xyz = _device_f64(xyz, "xyz")
    tt = torch.cat([_device_f64(xyz_tower1, "xyz_tower1"), _device_f64(xyz_tower2, "xyz_tower2")])
    lo, hi = tt.min(dim=0).values, tt.max(dim=0).values
    box = torch.stack([lo[0], lo[1], hi[0], hi[1]])[None]
    kinds = torch.full((1,), SN_CROP_BOX, dtype=torch.int32, device=xyz.device)
    crops = crop_regions(xyz, box, kinds, classes, want_src=False)
    return crops.pts, crops.labels.to(torch.int64)


def crop_tower_samples(xyz: torch.Tensor, classes: torch.Tensor, towers: Optional[Sequence[torch.Tensor]] = None,
                       radius: float = 15, obj_class=(15,), eps: float = 10, min_points: int = 300) -> List[torch.Tensor]:
    """pcd_processing.py:805-817: one [n_k, 4] sample (x, y, z, class) per tower, all cut in one pass.  towers None (the
    reference's own signature): the towers are found on the device as the reference finds them -- the points whose class
    is one of obj_class, clustered by DBSCAN(eps, min_points) (clusters.cluster_points).  towers given as a list of point
    sets: those are taken, and obj_class / eps / min_points are not read.  Tower means as in crop_tower_radius."""
    if towers is None:
        from .clusters import cluster_points
        xyz = _device_f64(xyz, "xyz")
        towers = cluster_points(xyz, eps, min_points, labels=_device_f64(classes, "classes"), keep=obj_class).towers()
    if len(towers) == 0:
        return []
    xyz = _device_f64(xyz, "xyz")
    rows = torch.cat([_tower_disc(t, radius) for t in towers])
    crops = crop_regions(xyz, rows, None, classes, want_src=False)
    return [torch.cat([p, l[:, None]], dim=1) for p, l in _tiles(crops)]


# --------------------------------------------------------------------------- #
def lattice_boxes(lo_xy: Sequence[float], hi_xy: Sequence[float], tile: float, overlap: float = 0.0) -> np.ndarray:
    """The rows of lattice_regions as a host array [K, 4] (xmin, ymin, xmax, ymax)."""
    lo = np.asarray(lo_xy, dtype=np.float64).reshape(2)
    hi = np.asarray(hi_xy, dtype=np.float64).reshape(2)
    tile, overlap = float(tile), float(overlap)
    if not (tile > 0 and overlap >= 0 and np.all(hi >= lo)):
        raise ValueError("lattice_regions needs tile > 0, overlap >= 0 and hi_xy >= lo_xy")
    counts = [max(1, int(np.ceil((hi[a] - lo[a]) / tile))) for a in range(2)]
    rows = []
    for ix in range(counts[0]):
        for iy in range(counts[1]):
            x0, y0 = lo[0] + ix * tile, lo[1] + iy * tile
            x1 = hi[0] if ix == counts[0] - 1 else lo[0] + (ix + 1) * tile
            y1 = hi[1] if iy == counts[1] - 1 else lo[1] + (iy + 1) * tile
            rows.append([max(lo[0], x0 - overlap), max(lo[1], y0 - overlap), min(hi[0], x1 + overlap),
                         min(hi[1], y1 + overlap)])
    return np.array(rows, dtype=np.float64)


def lattice_regions(lo_xy: Sequence[float], hi_xy: Sequence[float], tile: float, overlap: float = 0.0, device=None
                    ) -> Tuple[torch.Tensor, torch.Tensor]:
    """(regions [K,4] f64, kinds [K] int32) of boxes that cover the rectangle lo_xy .. hi_xy: cells of `tile` x `tile` on
    a lattice from lo_xy, row-major in (x, y), each grown by `overlap` on every side (neighbours share 2 * overlap) and
    clipped to the rectangle.  Host arithmetic (lattice_boxes), device tensors.  Boxes are inclusive, so with overlap 0 a
    point exactly on an inner lattice line belongs to both neighbours."""
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if device.type != "cuda":
        raise HipLibraryError("lattice_regions: the regions live on a HIP device; there is no CPU path")
    rows = lattice_boxes(lo_xy, hi_xy, tile, overlap)
    regions = torch.from_numpy(rows).to(device)
    return regions, torch.full((rows.shape[0],), SN_CROP_BOX, dtype=torch.int32, device=device)


def merge_to_scan(values: torch.Tensor, src: torch.Tensor, n: int, fill: float = 0.0) -> torch.Tensor:
    """values [total] (one per cropped row), src [total] int64 -> [n]: for every scan point the maximum over the tiles
    that hold it (scatter_reduce amax: deterministic), `fill` where none does."""
    if not values.is_cuda or not src.is_cuda:
        raise HipLibraryError("merge_to_scan: values and src must live on a HIP device; there is no CPU path")
    values = values.reshape(-1)
    if values.numel() != src.numel():
        raise ValueError("values and src disagree in length")
    out = torch.full((int(n),), float("-inf"), dtype=values.dtype, device=values.device)
    out.scatter_reduce_(0, src, values, reduce="amax", include_self=True)
    seen = torch.zeros((int(n),), dtype=torch.bool, device=values.device)
    seen[src] = True
    return torch.where(seen, out, torch.full_like(out, fill))
