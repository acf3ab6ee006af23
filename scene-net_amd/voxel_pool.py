"""Pooling points onto the voxel grid on the device (sn_voxel_pool, csrc/voxel_pool.hip): per voxel the mean, minimum or
maximum of a coordinate or of a per-point value column, and the voxel filter and the reference's centroid grids built on it.

    vp = sna.voxel_pool(batch, (64, 64, 64), planes=("z.mean", "z.min", "z.max", "v0.mean"), values=feat, value_ranges=[(0, 1)])
    cen = sna.voxel_centroids(batch, (64, 64, 64))                  # VoxelPool: planes [B,3,nz,nx,ny] f64, counts, desc, ...
    back = sna._hip.gather_points(cen.planes, batch.pts, batch.offsets, cen.desc)      # every point gets its voxel's centroid
    small, n = sna.voxel_downsample(batch, (64, 64, 64), label_rule="max")             # one row per occupied voxel
    g = sna.centroid_hist_on_voxel(xyz)                             # numpy [4,nz,nx,ny]: centroid x, y, z, then the density

The reference's xyz_Voxelization (core/datasets/torch_transforms.py:157-166) calls Vox.centroid_hist_on_voxel and
Vox.centroid_reg_on_voxel, which its tree does not contain; what is built here is the evident intent -- the mean position of
each voxel's points next to hist_on_voxel's density and reg_on_voxel's ratio, empty voxels 0 -- and is this build's reading,
not a mirror.

Definition (normative, include/scenenet_hip.h, K24).  The binning is K1's.  A mean is a FIXED-POINT mean: every input is
quantised to 2^-32 of its range (a coordinate's range is its tile's box in the descriptor, a value column's is
`value_ranges`), the quanta are summed as integers and the sum is decoded -- within span * 2^-33 of the fp64 mean of the
inputs clamped to the range, and bit-identical under any scheduling and any order of the rows.  Minima and maxima are by
value, as their 64-bit patterns.  A row with a NaN coordinate or outside the table is counted in `unbinned`, a binned row with
a NaN in a value column some plane reads in `nan_rows`; neither takes part in anything else.
There is no CPU path: CPU tensors raise HipLibraryError.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _hip
from . import voxelization as Vox
from ._hip import HipLibraryError
from .voxelization import PointBatch

_OPS = {"mean": _hip.SN_POOL_MEAN, "min": _hip.SN_POOL_MIN, "max": _hip.SN_POOL_MAX}
_AXES = {"x": 0, "y": 1, "z": 2}
CENTROID_PLANES = ("x.mean", "y.mean", "z.mean")


@dataclass
class VoxelPool:
    """What one voxel_pool call leaves on the device.
      planes   [B,P,nz,nx,ny] f64: plane p is names[p]; `fill` where counts == 0
      counts   [B,nz,nx,ny] int32: the rows that took part
      unbinned [B] int64: rows with a NaN coordinate or outside the table
      nan_rows [B] int64: binned rows with a NaN in a value column some plane reads
      desc     [B, desc_len] f64: the descriptor the rows were binned with (what sn_gather_points reads the planes back by)
      names    the planes' names as given
      dims     [B,3] int32 | None: each tile's own (n_x, n_y, n_z) in the voxel-size mode (the grid is the maximum's)"""
    planes: torch.Tensor
    counts: torch.Tensor
    unbinned: torch.Tensor
    nan_rows: torch.Tensor
    desc: torch.Tensor
    names: Tuple[str, ...]
    dims: Optional[torch.Tensor] = None


def parse_planes(planes: Sequence[str], C: int):
    """("x.mean", "v0.max", ...) -> (sources, ops) as sn_voxel_pool takes them."""
    sources, ops = [], []
    for name in planes:
        head, _, tail = str(name).partition(".")
        if tail not in _OPS:
            raise ValueError(f"plane '{name}': the reduction must be one of .mean, .min, .max")
        if head in _AXES:
            s = _AXES[head]
        elif head[:1] == "v" and head[1:].isdigit():
            s = 3 + int(head[1:])
            if s >= 3 + C:
                raise ValueError(f"plane '{name}' reads value column {s - 3}, values has {C}")
        else:
            raise ValueError(f"plane '{name}': the source must be x, y, z or v<column>")
        sources.append(s)
        ops.append(_OPS[tail])
    if not 1 <= len(sources) <= _hip.SN_POOL_MAX_PLANES:
        raise ValueError(f"1 .. {_hip.SN_POOL_MAX_PLANES} planes per call (got {len(sources)})")
    return sources, ops


def _ranges_on_device(values: torch.Tensor, columns: Sequence[int]):
    """(lo, hi) of each column's finite values, one host read; a column with none, or with one value only, is widened so that
    hi > lo."""
    if torch.cuda.is_current_stream_capturing():
        raise HipLibraryError("voxel_pool: value_ranges=None reads the columns' extrema back to the host, which a stream "
                              "capture cannot do; give value_ranges explicitly")
    C = int(values.shape[1])
    fin = torch.isfinite(values)
    big = torch.finfo(torch.float64).max
    lo = torch.where(fin, values, torch.full_like(values, big)).amin(dim=0)
    hi = torch.where(fin, values, torch.full_like(values, -big)).amax(dim=0)
    both = torch.stack([lo, hi]).cpu().numpy()
    out = [(0.0, 1.0)] * C
    for c in columns:
        a, b = float(both[0, c]), float(both[1, c])
        if a > b:                   # no finite value
            a, b = 0.0, 1.0
        if not b > a:
            b = a + max(1.0, abs(a))
        out[c] = (a, b)
    return out


def _descriptor(batch: PointBatch, n_xyz, desc, voxel_dims):
    dims = None
    if desc is not None:
        if voxel_dims is not None:
            raise ValueError("desc and voxel_dims are mutually exclusive")
        if isinstance(desc, np.ndarray):
            desc = torch.from_numpy(np.ascontiguousarray(desc, dtype=np.float64)).to(batch.pts.device)
        if not isinstance(desc, torch.Tensor) or not desc.is_cuda:
            raise HipLibraryError("desc must live on a HIP device; there is no CPU path")
        desc = desc.to(torch.float64).contiguous()
    elif voxel_dims is not None:
        bbox = _hip.voxel_bbox(batch.pts, batch.offsets)
        desc, dims, _ = _hip.voxel_desc_sized(bbox, voxel_dims, n_xyz)
    else:
        desc, _ = _hip.voxel_prepare(batch.pts, batch.offsets, n_xyz, regular=True)
    return desc, dims


def voxel_pool(batch: PointBatch, voxelgrid_dims: Sequence[int] = (64, 64, 64), planes: Sequence[str] = CENTROID_PLANES,
               values: Optional[torch.Tensor] = None, value_ranges: Optional[Sequence[Sequence[float]]] = None,
               desc: Optional[torch.Tensor] = None, fill: float = 0.0,
               voxel_dims: Optional[Sequence[float]] = None) -> VoxelPool:
    """Up to eight planes per voxel of every tile (module docstring).
      voxelgrid_dims  (x, y, z) like the reference; the planes come back [B,P,nz,nx,ny]
      planes          names "x|y|z|v<c>" + ".mean|.min|.max"; a source may appear in several
      values          [total,C] (or [total]) on the device, C <= 5: the per-point channels the v<c> planes read
      value_ranges    [C] pairs (lo, hi): the range a MEAN plane quantises column c over (values beyond it, +-inf included,
                      count as its ends).  None: each such column's finite minimum and maximum, taken on the device and read
                      back -- ONE host read; under a stream capture that raises, give the ranges.
      desc            None: the descriptor sna.voxel_classes builds for the same arguments (the cube of each tile, or the
                      size-mode tables with `voxel_dims`, `voxelgrid_dims` then the maximum).  Given [B, desc_len]: the rows
                      are binned with it, foreign or not.
      fill            what an empty voxel holds in every plane (its bit pattern is kept)
    With explicit ranges: no synchronisation, nothing is read back."""
    if not isinstance(batch, PointBatch):
        raise ValueError("voxel_pool takes a PointBatch")
    if not batch.pts.is_cuda:
        raise HipLibraryError("the batch must live on a HIP device; there is no CPU path")
    if int(batch.pts.shape[0]) == 0:
        raise ValueError("voxel_pool needs at least one point")
    nx, ny, nz = (int(v) for v in voxelgrid_dims)
    dev = batch.pts.device
    B = int(batch.offsets.numel()) - 1
    C = 0
    if values is not None:
        if not isinstance(values, torch.Tensor) or not values.is_cuda:
            raise HipLibraryError("values must live on a HIP device; there is no CPU path")
        values = values.to(torch.float64)
        values = (values.reshape(-1, 1) if values.dim() == 1 else values).contiguous()
        C = int(values.shape[1])
        if C > _hip.SN_POOL_MAX_COLUMNS:
            raise ValueError(f"at most {_hip.SN_POOL_MAX_COLUMNS} value columns per call (got {C})")
    sources, ops = parse_planes(planes, C)
    mean_cols = sorted({s - 3 for s, o in zip(sources, ops) if s >= 3 and o == _hip.SN_POOL_MEAN})
    if value_ranges is None and mean_cols:
        value_ranges = _ranges_on_device(values, mean_cols)
    elif value_ranges is not None:
        value_ranges = [(float(a), float(b)) for a, b in value_ranges]
        if len(value_ranges) != C:
            raise ValueError(f"value_ranges must hold one (lo, hi) per value column: {C} (got {len(value_ranges)})")
        for c in mean_cols:
            a, b = value_ranges[c]
            if not (math.isfinite(a) and math.isfinite(b) and b > a):
                raise ValueError(f"value_ranges[{c}] must be finite with hi > lo (got {a}, {b})")
    desc, dims = _descriptor(batch, (nx, ny, nz), desc, voxel_dims)
    P = len(sources)
    out = torch.empty((B, P, nz, nx, ny), dtype=torch.float64, device=dev)
    counts = torch.empty((B, nz, nx, ny), dtype=torch.int32, device=dev)
    unbinned = torch.empty((B,), dtype=torch.int64, device=dev)
    nan_rows = torch.empty((B,), dtype=torch.int64, device=dev)
    _hip.voxel_pool(batch.pts, values, batch.offsets, desc, (nx, ny, nz), sources, ops, value_ranges, fill, out, counts,
                    unbinned, nan_rows)
    return VoxelPool(out, counts, unbinned, nan_rows, desc, tuple(str(p) for p in planes), dims)


def voxel_centroids(batch: PointBatch, voxelgrid_dims: Sequence[int] = (64, 64, 64),
                    desc: Optional[torch.Tensor] = None) -> VoxelPool:
    """The mean position of every voxel's points: planes [B,3,nz,nx,ny] = (x, y, z), 0 where no point fell."""
    return voxel_pool(batch, voxelgrid_dims, CENTROID_PLANES, desc=desc)


def _centroids_next_to(xyz, labels, tower_label, voxelgrid_dims, voxel_dims, want_density: bool, want_gt: bool):
    """One tile's centroid planes [3,nz,nx,ny] and its VoxelGrids, every channel binned by ONE table: the descriptor the
    density / ratio call returns is the one the centroids are pooled with, and a size-mode grid is cut as
    voxelization._voxelize_single cuts it."""
    batch = PointBatch.from_tiles([xyz], None if labels is None else [labels])
    g = Vox._voxelize_single(batch.pts, batch.labels, tower_label, voxelgrid_dims, voxel_dims, want_density=want_density,
                             want_gt=want_gt, want_occ=False)
    ref = g.density if g.density is not None else g.gt
    nz, nx, ny = (int(v) for v in ref.shape[-3:])
    if g.dims is not None:        # size mode within the capacity: the padded table, then the tile's own corner of the grid
        table = tuple(max(int(v), 1) for v in voxelgrid_dims)
    else:
        table = (nx, ny, nz)
    vp = voxel_pool(batch, table, CENTROID_PLANES, desc=g.desc, fill=0.0)
    return vp.planes[0, :, :nz, :nx, :ny], g


def centroid_hist_on_voxel(xyz, voxelgrid_dims=(64, 64, 64), voxel_dims=None) -> np.ndarray:
    """This build's reading of the function torch_transforms.py:161 calls: [4,nz,nx,ny] f64 = the centroid planes x, y, z (0
    in an empty voxel), then hist_on_voxel's density."""
    cen, g = _centroids_next_to(xyz, None, None, voxelgrid_dims, voxel_dims, True, False)
    return torch.cat([cen, g.density[0]]).cpu().numpy()


def centroid_reg_on_voxel(xyz, labels, tower_label, voxelgrid_dims=(64, 64, 64), voxel_dims=None) -> np.ndarray:
    """This build's reading of the function torch_transforms.py:162 calls: [4,nz,nx,ny] f64 = the centroid planes x, y, z,
    then reg_on_voxel's ratio."""
    cen, g = _centroids_next_to(xyz, labels, tower_label, voxelgrid_dims, voxel_dims, False, True)
    return torch.cat([cen, g.gt[0]]).cpu().numpy()


def voxel_downsample(batch: PointBatch, voxelgrid_dims: Sequence[int] = (64, 64, 64), desc: Optional[torch.Tensor] = None,
                     label_rule: Optional[str] = None):
    """The voxel-grid filter: one row per occupied voxel, at the centroid of its points, in flat [z][x][y] voxel order per
    tile.  label_rule None: no labels; "max": the largest label of the voxel that is not NaN (sna.voxel_classes, K18).
    -> (PointBatch, counts [rows] int32: how many points each row stands for).
    The compaction is torch.nonzero on the counts: the sizes are read back to the host, so the call is NOT capturable.  It is
    for tiles whose dense grid fits; a tile none of whose rows is binned comes back empty."""
    if label_rule not in (None, "max"):
        raise ValueError("label_rule must be None or 'max'")
    if label_rule == "max" and batch.labels is None:
        raise ValueError("label_rule='max' needs the batch's labels")
    vp = voxel_pool(batch, voxelgrid_dims, CENTROID_PLANES, desc=desc)
    B = int(vp.counts.shape[0])
    flat = vp.counts.reshape(B, -1)
    where = torch.nonzero(flat)                                   # [rows, 2] in (tile, voxel) order
    tile, voxel = where[:, 0], where[:, 1]
    pts = vp.planes.reshape(B, 3, -1)[tile, :, voxel].contiguous()
    labels = None
    if label_rule == "max":
        from .voxel_classes import voxel_classes
        labels = voxel_classes(batch, voxelgrid_dims, desc=vp.desc).grid.reshape(B, -1)[tile, voxel].contiguous()
    sizes = torch.bincount(tile, minlength=B)
    offsets = torch.cat([sizes.new_zeros(1), torch.cumsum(sizes, 0)])
    return (PointBatch(pts, labels, offsets, tuple(int(v) for v in sizes.cpu()), batch.tile_ids),
            flat[tile, voxel].contiguous())
