"""Semantic voxel grids and class colours on the device (sn_voxel_classes / sn_class_census / sn_class_paint,
csrc/voxel_classes.hip).

The reference builds a per-voxel class grid on the host (utils/voxelization.py:207-241, classes_on_voxel: a pandas
groupby(["z", "x", "y"]).max() over the points' labels and a Python loop over the occupied voxels) and a scan's class colours
with a Python loop over every point (utils/pcd_processing.py:525-574, color_pointcloud: np.unique(classes), then
class_color[np.where(unique_classes == c)[0][0]] per point).  Here both stay in HBM:

    vc = sna.voxel_classes(batch)                              # VoxelClasses: grid [B,1,nz,nx,ny] f64, desc, unbinned, ...
    coarse = sna._hip.gather_points(vc.grid, batch.pts, batch.offsets, vc.desc)        # the class map painted back
    grid = sna.classes_on_voxel(xyz, labels)                   # the reference's call: numpy [nz,nx,ny]
    cc = sna.class_colors(classes, table, las=True)            # ClassColors: rgb [n,3] u16 for sna.write_las(..., rgb=cc.rgb)
    colors = sna.color_pointcloud(None, classes, class_color=table)                    # the reference's call, a device tensor

Grid (normative, include/scenenet_hip.h): a voxel no binned row falls in holds +0.0, one whose binned rows all carry NaN
labels holds NaN, any other the largest label that is not NaN -- pandas' max.  The binning is K1's.  Unpinned, as for K1 and
K17: pyntcloud's own binning (not installed here); the voxels are K1's, checked against its oracle.
Colours: a class is VALID iff it is integral and in 0 .. 65535; a row's colour is table[rank of its class among the tile's
valid classes] -- np.unique's index.  A row that is not valid, or whose rank the table does not reach, is counted (`bad`,
`short_table`) and gets a NaN colour; the reference raises IndexError for it, and so does color_pointcloud here.
There is no CPU path: CPU tensors raise HipLibraryError.
"""
from __future__ import annotations

import pickle
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np
import torch

from . import _hip
from ._hip import HipLibraryError
from .voxelization import PointBatch, _device_f64


@dataclass
class VoxelClasses:
    """What one voxel_classes call leaves on the device.
      grid       [B,1,nz,nx,ny] f64: the largest label of every voxel (0 where empty, NaN where only NaN labels fell)
      desc       [B, desc_len] f64: the descriptor the rows were binned with (what sn_gather_points reads the grid back by)
      unbinned   [B] int64: rows with a NaN coordinate or outside the table
      nan_labels [B] int64: rows whose label is NaN
      dims       [B,3] int32 | None: each tile's own (n_x, n_y, n_z) in the voxel-size mode (the grid is the maximum's)"""
    grid: torch.Tensor
    desc: torch.Tensor
    unbinned: torch.Tensor
    nan_labels: torch.Tensor
    dims: Optional[torch.Tensor] = None


@dataclass
class ClassColors:
    """What one class_colors call leaves on the device.
      colors      [total,3] f64 | None: table[rank of the row's class]; NaN for a row that has no colour
      rgb         [total,3] uint16 | None (las=True): clamp(rint(255 c), 0, 255) * 257; zeros for a row that has no colour
      unique      [B, U_max] f64: each tile's valid classes in ascending order in its first n_unique[b] slots, NaN behind them
      n_unique    [B] int64
      bad         [B] int64: rows that are not a valid class (NaN, fractional, negative, above 65535)
      short_table [B] int64: rows whose class's rank is beyond the table"""
    colors: Optional[torch.Tensor]
    rgb: Optional[torch.Tensor]
    unique: torch.Tensor
    n_unique: torch.Tensor
    bad: torch.Tensor
    short_table: torch.Tensor


def voxel_classes(batch: PointBatch, voxelgrid_dims: Sequence[int] = (64, 64, 64), desc: Optional[torch.Tensor] = None,
                  voxel_dims: Optional[Sequence[float]] = None) -> VoxelClasses:
    """classes_on_voxel for a whole batch: the largest label of every voxel of every tile (module docstring).
      voxelgrid_dims  (x, y, z) like the reference; the grid comes back [B,1,nz,nx,ny]
      desc            None: the descriptor voxelize_batch builds for the same arguments (sn_voxel_prepare with the regular
                      box, or sn_voxel_bbox + sn_voxel_desc_sized with `voxel_dims`, `voxelgrid_dims` then the maximum).
                      Given [B, desc_len]: the rows are binned with it, foreign or not -- a crop's labels go into the grid of
                      the tile it was cut from.  Rows it does not hold are counted in `unbinned`.
    No synchronisation, nothing is read back."""
    if not isinstance(batch, PointBatch):
        raise ValueError("voxel_classes takes a PointBatch")
    if not batch.pts.is_cuda:
        raise HipLibraryError("the batch must live on a HIP device; there is no CPU path")
    if batch.labels is None:
        raise ValueError("voxel_classes needs the batch's labels")
    nx, ny, nz = (int(v) for v in voxelgrid_dims)
    dev = batch.pts.device
    B = int(batch.offsets.numel()) - 1
    if int(batch.pts.shape[0]) == 0:
        raise ValueError("voxel_classes needs at least one point")
    dims = None
    if desc is not None:
        if voxel_dims is not None:
            raise ValueError("desc and voxel_dims are mutually exclusive")
        desc = _device_f64(desc, "desc", numpy_ok=True)
    elif voxel_dims is not None:
        bbox = _hip.voxel_bbox(batch.pts, batch.offsets)
        desc, dims, _ = _hip.voxel_desc_sized(bbox, voxel_dims, (nx, ny, nz))
    else:
        desc, _ = _hip.voxel_prepare(batch.pts, batch.offsets, (nx, ny, nz), regular=True)
    grid = torch.empty((B, 1, nz, nx, ny), dtype=torch.float64, device=dev)
    unbinned = torch.empty((B,), dtype=torch.int64, device=dev)
    nan_labels = torch.empty((B,), dtype=torch.int64, device=dev)
    _hip.voxel_classes(batch.pts, batch.labels, batch.offsets, desc, (nx, ny, nz), grid, unbinned, nan_labels)
    return VoxelClasses(grid, desc, unbinned, nan_labels, dims)


def classes_on_voxel(xyz, labels, voxel_dims: Sequence[int] = (64, 64, 64)) -> np.ndarray:
    """voxelization.py:207-241 (there `voxel_dims` names the GRID's dims): per-voxel largest label -> [nz,nx,ny] f64."""
    batch = PointBatch.from_tiles([xyz], [labels])
    return voxel_classes(batch, voxel_dims).grid[0, 0].cpu().numpy()


def class_colors(classes, class_color, offsets: Optional[torch.Tensor] = None, las: bool = False,
                 max_unique: Optional[int] = None) -> ClassColors:
    """Each row's colour by its class's rank among its tile's classes (module docstring).
      classes      [total] on the device (any real dtype; taken as f64), or a numpy array (copied up)
      class_color  [T,3] table (numpy or device tensor), row k the colour of the tile's k-th smallest class
      offsets      [B+1] int64 on the device: a CSR batch of class vectors, every tile ranked by its own classes; None: one
                   tile, the whole vector
      las          False: colors [total,3] f64.  True: rgb [total,3] uint16, what sna.write_las takes
      max_unique   columns of `unique` (default: the table's rows, where a table that serves reaches)
    Everything stays on the device; nothing is read back."""
    cls = _device_f64(classes, "classes", numpy_ok=True).reshape(-1)
    dev = cls.device
    total = int(cls.numel())
    if total == 0:
        raise ValueError("class_colors needs at least one row")
    table = _device_f64(class_color, "class_color", numpy_ok=True)
    if table.dim() != 2 or table.shape[1] != 3 or table.shape[0] < 1:
        raise ValueError(f"class_color must be [T, 3] with T >= 1 (got {tuple(table.shape)})")
    if offsets is None:
        offsets = torch.tensor([0, total], dtype=torch.int64, device=dev)
    elif not isinstance(offsets, torch.Tensor) or not offsets.is_cuda:
        raise HipLibraryError("offsets must live on a HIP device; there is no CPU path")
    B = int(offsets.numel()) - 1
    U = int(table.shape[0]) if max_unique is None else int(max_unique)
    present = torch.empty((B, _hip.SN_CLASS_WORDS), dtype=torch.int32, device=dev)
    bad = torch.empty((B,), dtype=torch.int64, device=dev)
    n_unique = torch.empty((B,), dtype=torch.int64, device=dev)
    short_table = torch.empty((B,), dtype=torch.int64, device=dev)
    unique = torch.full((B, U), float("nan"), dtype=torch.float64, device=dev)
    colors = None if las else torch.empty((total, 3), dtype=torch.float64, device=dev)
    rgb = torch.empty((total, 3), dtype=torch.uint16, device=dev) if las else None
    _hip.class_census(cls, offsets, present, bad)
    _hip.class_paint(cls, offsets, present, table, colors, rgb, unique, n_unique, short_table)
    return ClassColors(colors, rgb, unique, n_unique, bad, short_table)


def random_class_colors(n_classes: int) -> np.ndarray:
    """[n_classes,3] f64: the reference's own draw (pcd_processing.py:559-560) from numpy's global generator."""
    return np.random.choice(256, size=(int(n_classes), 3)) / 255


def color_pointcloud(pcd, classes, load: bool = False, pck_name: str = "class_colors", class_color=None):
    """pcd_processing.py:525-574 with the classes on the device: -> [n,3] f64 on the device, row i = class_color[index of
    classes[i] in np.unique(classes)].  load=True returns the pickle `pck_name` as the reference does.  class_color None: the
    set of classes is read back (one 8 KiB copy) and the table drawn on the host by the reference's own call, so a seeded
    numpy gives the reference's table.  A class that is not an integer in 0 .. 65535, or a table with fewer rows than there
    are classes, raises IndexError (the reference's own error for a NaN and a short table).  `pcd` may be None; otherwise its
    `.colors` is set to the result."""
    if load:
        with open(pck_name, "rb") as handle:
            np_colors = pickle.load(handle)
    else:
        cls = _device_f64(classes, "classes", numpy_ok=True).reshape(-1)
        dev = cls.device
        total = int(cls.numel())
        if total == 0:
            np_colors = torch.empty((0, 3), dtype=torch.float64, device=dev)
        elif class_color is None:
            offsets = torch.tensor([0, total], dtype=torch.int64, device=dev)
            present = torch.empty((1, _hip.SN_CLASS_WORDS), dtype=torch.int32, device=dev)
            bad = torch.empty((1,), dtype=torch.int64, device=dev)
            n_unique = torch.empty((1,), dtype=torch.int64, device=dev)
            short_table = torch.empty((1,), dtype=torch.int64, device=dev)
            _hip.class_census(cls, offsets, present, bad)
            # the one read-back: the tile's bitmap (8 KiB), whose set bits are the classes; rank and paint wait for the table
            n = int(np.unpackbits(present.cpu().numpy().view(np.uint8)).sum())
            table = torch.from_numpy(random_class_colors(n if n > 0 else 1)).to(dev)
            np_colors = torch.empty((total, 3), dtype=torch.float64, device=dev)
            _hip.class_paint(cls, offsets, present, table, np_colors, None, None, n_unique, short_table)
            _raise_on_rows(bad, short_table)
        else:
            cc = class_colors(cls, class_color)
            _raise_on_rows(cc.bad, cc.short_table)
            np_colors = cc.colors
    if pcd is not None:
        pcd.colors = np_colors
    return np_colors


def _raise_on_rows(bad: torch.Tensor, short_table: torch.Tensor) -> None:
    nbad, nshort = (int(v) for v in torch.stack([bad.sum(), short_table.sum()]).cpu())
    if nbad:
        raise IndexError(f"{nbad} rows hold no valid class (an integer in 0 .. 65535): index 0 is out of bounds for axis 0 "
                         "with size 0")
    if nshort:
        raise IndexError(f"{nshort} rows hold a class beyond the table's rows: index is out of bounds for axis 0")
