"""Coloured voxel clouds on the device: the non-zero voxels of a batch of grids as rows (x, y, z, r, g, b)
(sn_voxel_cloud_count / sn_voxel_cloud_scatter, csrc/voxel_cloud.hip).

The reference turns a grid into something a person looks at with plot_voxelgrid(grid, color_mode, plot=False)
(utils/voxelization.py:45-144, color_pointcloud of utils/pcd_processing.py:525-574 behind it): a Python loop over
grid.nonzero() and an np.where per voxel, on the host, after a .detach().cpu().numpy() -- three times per logged batch in
LitSceneNet.on_validation_batch_end (core/lit_modules/lit_model_wrappers.py:222-233).  Here a batch of grids that stays in
HBM becomes a CSR batch of clouds in four launches:

    cloud = sna.voxel_cloud(pred, 'ranges', desc=grids.desc)       # VoxelCloud: rows | xyz + rgb, offsets, bad
    rows_b = cloud.tile(b)                                          # [n_b, 6] f64, the reference's rows for grid b
    sna.write_voxel_cloud_las("pred.las", sna.voxel_cloud(pred, 'ranges', desc=grids.desc, las=True), k=0)

Definition (normative, include/scenenet_hip.h): grid [Z, X, Y], a value read as fp64; one row per voxel with value != 0
in C order of (z, x, y), the row (x, y, z, 255 r, 255 g, 255 b).  density: c < 0 -> (1 + c, 1 + c, 1), otherwise
(1, 1 - c, 1 - c).  ranges: lin = np.linspace(0, 1, r), step = (1 / r) / 2, a row is kept iff value > lin[1] and its colour
is row argmin_j |(value - lin[j]) - step| of jet_ranges(r).  With `desc` (build-defined) x, y, z are the voxel centres in
scan coordinates and a size-mode tile's padding cells are left out.
There is no CPU path: CPU tensors raise HipLibraryError.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple, Union

import numpy as np
import torch

from . import _hip
from ._hip import SN_CLOUD_DENSITY, SN_CLOUD_MAX_R, SN_CLOUD_RANGES, HipLibraryError

_MODES = {"density": SN_CLOUD_DENSITY, "ranges": SN_CLOUD_RANGES}

# matplotlib.cm.jet(np.linspace(0, 1, 10))[:, :3] with row 0 forced to white (the reference's default r), as literals: the
# package needs no matplotlib at run time
_JET_10 = (
    (1.0, 1.0, 1.0),
    (0.0, 0.0, 0.999108734402852),
    (0.0, 0.3784313725490196, 1.0),
    (0.0, 0.8333333333333334, 1.0),
    (0.30044275774826057, 1.0, 0.6672991777356103),
    (0.6672991777356103, 1.0, 0.30044275774826057),
    (1.0, 0.9012345679012348, 0.0),
    (1.0, 0.48002904865649987, 0.0),
    (0.9991087344028523, 0.07334785766158336, 0.0),
    (0.5, 0.0, 0.0),
)


def jet_ranges(r: int = 10) -> np.ndarray:
    """The `ranges` colour table [r, 3] f64: cm.jet(np.linspace(0, 1, r))[:, :3] with row 0 forced to (1, 1, 1)
    (utils/voxelization.py:113-116).  r == 10 is embedded; another r needs matplotlib."""
    r = int(r)
    if not 2 <= r <= SN_CLOUD_MAX_R:
        raise ValueError(f"r must be in 2..{SN_CLOUD_MAX_R} (got {r})")
    if r == 10:
        return np.array(_JET_10, dtype=np.float64)
    try:
        import matplotlib.cm as cm
    except ImportError as e:
        raise ValueError(f"the jet table for r={r} needs matplotlib (only r=10 is embedded): pass color_ranges") from e
    table = np.array(cm.jet(np.linspace(0, 1, r)), dtype=np.float64)[:, :3].copy()
    table[0] = 1.0
    return table


def _table(mode: str, r: int, color_ranges) -> Optional[np.ndarray]:
    if mode != "ranges":
        return None
    if color_ranges is None:
        return jet_ranges(r)
    table = np.asarray(color_ranges, dtype=np.float64)
    if table.ndim != 2 or table.shape[0] != r or table.shape[1] not in (3, 4):
        raise ValueError(f"color_ranges must be [r, 3] (or [r, 4], the alpha dropped) with r={r} (got {table.shape})")
    return np.ascontiguousarray(table[:, :3])


@dataclass
class VoxelCloud:
    """What one voxel_cloud call leaves on the device: a CSR batch of B clouds.
      rows    [total | capacity, 6] f64 (x, y, z, 255 r, 255 g, 255 b) | None
      xyz     [.., 3] f64 and rgb [.., 3] uint16 (clamp(rint(255 c), 0, 255) * 257) | None: the LAS writer's form
      offsets [B+1] int64: the TRUE sizes, also where a given capacity was too small
      bad     [B, 2] int64: (NaN voxels kept, voxels whose colour left [0, 255]) -- density only"""
    rows: Optional[torch.Tensor]
    xyz: Optional[torch.Tensor]
    rgb: Optional[torch.Tensor]
    offsets: torch.Tensor
    bad: torch.Tensor
    color_mode: str

    @property
    def B(self) -> int:
        return int(self.offsets.numel()) - 1

    @property
    def capacity(self) -> int:
        return int((self.rows if self.rows is not None else self.xyz).shape[0])

    def sizes(self):
        """Rows per cloud (copies offsets to the host: synchronises)."""
        return tuple(int(v) for v in np.diff(self.offsets.cpu().numpy()))

    def _span(self, k: int):
        lo, hi = (int(v) for v in self.offsets[k:k + 2].cpu())
        if hi > self.capacity:
            raise HipLibraryError(f"cloud {k} ends at row {hi}, beyond the capacity of {self.capacity} rows")
        return lo, hi

    def tile(self, k: int) -> Union[torch.Tensor, Tuple[torch.Tensor, torch.Tensor]]:
        """rows [n_k, 6] of cloud k, or (xyz [n_k, 3], rgb [n_k, 3]) in the LAS form: views (reads two offsets:
        synchronises)."""
        lo, hi = self._span(k)
        if self.rows is not None:
            return self.rows[lo:hi]
        return self.xyz[lo:hi], self.rgb[lo:hi]

    def check(self) -> None:
        """Raises ValueError when a NaN voxel was kept (the reference raises IndexError on one).  Synchronises."""
        nan = int(self.bad[:, 0].sum())
        if nan:
            raise ValueError(f"{nan} voxels are NaN: they have no colour (written as (255, NaN, NaN))")


def voxel_cloud(grids: torch.Tensor, color_mode: str = "density", r: int = 10, color_ranges=None,
                desc: Optional[torch.Tensor] = None, capacity: Optional[int] = None, las: bool = False) -> VoxelCloud:
    """grids [B, nz, nx, ny] or [B, 1, nz, nx, ny] (f32 | f64 | u8 | bool) on the device -> VoxelCloud (module docstring).
    desc: the voxelisation's descriptor (VoxelGrids.desc) -> voxel centres in scan coordinates.  las: xyz + rgb (uint16)
    instead of rows.  capacity None: count, ONE read of offsets[B] to the host, exact allocation, scatter.  capacity int:
    count and scatter back to back with no synchronisation (capturable); the outputs have `capacity` rows, rows beyond
    offsets[B] are uninitialised, and whether the clouds fit is the caller's to check from offsets[B]."""
    if color_mode not in _MODES:
        raise ValueError(f"color_mode must be in ['density', 'ranges']; got {color_mode}")
    if not isinstance(grids, torch.Tensor) or not grids.is_cuda:
        raise HipLibraryError("grids must live on a HIP device; there is no CPU path")
    if grids.dim() == 5 and grids.shape[1] == 1:
        grids = grids[:, 0]
    if grids.dim() != 4:
        raise ValueError(f"grids must be [B, nz, nx, ny] or [B, 1, nz, nx, ny] (got {tuple(grids.shape)})")
    if grids.dtype not in (torch.float32, torch.float64, torch.uint8, torch.bool):
        raise HipLibraryError(f"grids dtype {grids.dtype} unsupported (f32, f64, u8, bool)")
    if grids.numel() == 0:
        raise ValueError("voxel_cloud needs at least one grid with at least one voxel")
    r = int(r)
    if color_mode == "ranges" and not 2 <= r <= SN_CLOUD_MAX_R:
        raise ValueError(f"r must be in 2..{SN_CLOUD_MAX_R} (got {r})")
    table = _table(color_mode, r, color_ranges)
    if desc is not None and (not isinstance(desc, torch.Tensor) or not desc.is_cuda):
        raise HipLibraryError("desc must live on a HIP device; there is no CPU path")
    grids = grids.contiguous()
    mode = _MODES[color_mode]
    B, dev = int(grids.shape[0]), grids.device
    ws = torch.empty(_hip.voxel_cloud_ws_bytes(B, grids[0].numel()) // 8, dtype=torch.int64, device=dev)
    offsets = torch.empty(B + 1, dtype=torch.int64, device=dev)
    bad = torch.empty((B, 2), dtype=torch.int64, device=dev)
    _hip.voxel_cloud_count(grids, mode, r, desc, ws, offsets, bad)
    n = int(offsets[-1]) if capacity is None else int(capacity)
    if n < 0:
        raise ValueError("capacity must not be negative")
    rows = None if las else torch.empty((n, 6), dtype=torch.float64, device=dev)
    xyz = torch.empty((n, 3), dtype=torch.float64, device=dev) if las else None
    rgb = torch.empty((n, 3), dtype=torch.uint16, device=dev) if las else None
    if n > 0:   # (an empty buffer has no address to hand over, and nothing could be written to it)
        _hip.voxel_cloud_scatter(grids, mode, r, table, desc, ws, offsets, rows, xyz, rgb)
    return VoxelCloud(rows, xyz, rgb, offsets, bad, color_mode)


def _one_grid(grid) -> torch.Tensor:
    t = grid if isinstance(grid, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(grid))
    if t.dim() != 3:
        raise ValueError(f"plot_voxelgrid expects a 3-D grid, got shape {tuple(t.shape)}")
    if not t.is_cuda:
        t = t.to(torch.device("cuda", torch.cuda.current_device()))
    if t.dtype not in (torch.float32, torch.float64, torch.uint8, torch.bool):
        t = t.to(torch.float64)
    return t.detach()[None]


def plot_voxelgrid(grid, color_mode: str = "density", title: str = "VoxelGrid", visual: bool = False, plot: bool = True,
                   as_tensor: bool = False, **kwargs):
    """utils/voxelization.py:45-144 with the reference's signature; grid [Z, X, Y] as numpy or a tensor, on the host or
    the device (as vxg_to_xyz takes it: the work is done on the device).  plot=False returns what the reference returns:
    None for a grid without a non-zero voxel, a (0, 6) array for a `ranges` grid whose rows are all filtered out, otherwise
    the (N, 6) fp64 rows (x, y, z, 255 r, 255 g, 255 b) -- a numpy array, or the device tensor with `as_tensor`.
    kwargs: r (default 10) and color_ranges.  plot=True raises NotImplementedError: there is no GUI here.  An unknown
    color_mode raises ValueError (the reference builds that error and forgets to raise it); a NaN voxel in the density
    mode raises ValueError (the reference: IndexError)."""
    if color_mode not in _MODES:
        raise ValueError(f"color_mode must be in ['density', 'ranges']; got {color_mode}")
    if plot:
        raise NotImplementedError("plot_voxelgrid(plot=True) opens a viewer: there is none here; plot=False returns the rows")
    unknown = set(kwargs) - {"r", "color_ranges"}
    if unknown:
        raise TypeError(f"plot_voxelgrid got unexpected keyword arguments {sorted(unknown)}")
    t = _one_grid(grid)
    cloud = voxel_cloud(t, color_mode, kwargs.get("r", 10), kwargs.get("color_ranges"))
    n = int(cloud.rows.shape[0])
    if n == 0:
        # `ranges` dropped every row: None only if there was no non-zero voxel to begin with (the density count says)
        if color_mode == "density" or _nonzero_count(t) == 0:
            return None
        return cloud.rows if as_tensor else np.empty((0, 6))
    cloud.check()
    return cloud.rows if as_tensor else cloud.rows.cpu().numpy()


def _nonzero_count(grids: torch.Tensor) -> int:
    B, dev = int(grids.shape[0]), grids.device
    ws = torch.empty(_hip.voxel_cloud_ws_bytes(B, grids[0].numel()) // 8, dtype=torch.int64, device=dev)
    offsets = torch.empty(B + 1, dtype=torch.int64, device=dev)
    bad = torch.empty((B, 2), dtype=torch.int64, device=dev)
    _hip.voxel_cloud_count(grids.contiguous(), SN_CLOUD_DENSITY, 10, None, ws, offsets, bad)
    return int(offsets[-1])


def plot_quantile_uncertainty(vxg, legend: bool = False, as_tensor: bool = False):
    """utils/voxelization.py:147-155: the `ranges` rows of vxg[-1] - vxg[0] for vxg [Q, Z, X, Y], Q >= 2 (the reference
    opens a viewer on them; here they are returned)."""
    if len(vxg.shape) != 4:
        raise ValueError(f"Inadmissible shape: {tuple(vxg.shape)}")
    if vxg.shape[0] < 2:
        raise ValueError("the plot requires at least two quantile predictions")
    return plot_voxelgrid(vxg[-1] - vxg[0], color_mode="ranges", title="Aletoric Uncertainty through Quantiles",
                          visual=legend, plot=False, as_tensor=as_tensor)


def write_voxel_cloud_las(path: str, cloud: VoxelCloud, k: Optional[int] = None, **las_kw):
    """Sends a cloud made with las=True (xyz + rgb) through LasWriter: cloud k, or all of them with k None.  Point format 2
    unless given -- a prediction a viewer opens, in scan coordinates when the cloud was made with `desc`.  Returns
    LasWriter.write's LasWritten.  Synchronises."""
    from .las_write import write_las
    if cloud.xyz is None or cloud.rgb is None:
        raise HipLibraryError("write_voxel_cloud_las takes a cloud made with las=True (xyz + rgb)")
    if k is None:
        total = int(cloud.offsets[-1])
        if total > cloud.capacity:
            raise HipLibraryError(f"the clouds hold {total} rows, beyond the capacity of {cloud.capacity}")
        xyz, rgb = cloud.xyz[:total], cloud.rgb[:total]
    else:
        xyz, rgb = cloud.tile(k)
    las_kw.setdefault("point_format", 2)
    return write_las(path, xyz.contiguous(), rgb=rgb.contiguous(), **las_kw)
