"""Host-side mirror of the voxelisation step: utils/voxelization.py:164-204 (`hist_on_voxel`),
:244-300 (`reg_on_voxel`), :304-323 (`prob_to_label`) over eda.voxelize_ply
(utils/pcd_processing.py:341-372) / pyntcloud VoxelGrid.

`hist_on_voxel` / `reg_on_voxel` keep the reference's numpy-in / numpy-out signatures (host
buffers: PCIe-inclusive).  `voxelize_batch` is the HBM-resident form the fused pipeline and the
bench use: a ragged batch of tiles -> device grids in one pass of the HIP kernels
(csrc/voxel.hip).  No CPU path: everything below calls the C ABI.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _hip

ArrayLike = Union[np.ndarray, torch.Tensor]


@dataclass
class PointBatch:
    """Ragged batch of tiles resident in HBM: pts [total,3] f64, labels [total] f64 | None, offsets [B+1] i64.
    tile_ids [B] i64 | None: each tile's index in its dataset, where a loader knows it (what thin_points draws by)."""
    pts: torch.Tensor
    labels: Optional[torch.Tensor]
    offsets: torch.Tensor
    sizes: Tuple[int, ...]
    tile_ids: Optional[torch.Tensor] = None

    @property
    def batch(self) -> int:
        return len(self.sizes)

    @property
    def total_points(self) -> int:
        return int(sum(self.sizes))

    @staticmethod
    def from_tiles(tiles: Sequence[ArrayLike], labels: Optional[Sequence[ArrayLike]] = None,
                   device=None) -> "PointBatch":
        """Concatenates per-tile [N_b,3] arrays (numpy or torch, any device) into one CSR batch on the HIP device."""
        device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if device.type != "cuda":
            raise _hip.HipLibraryError("PointBatch lives in HBM: device must be a HIP device")
        sizes = tuple(int(t.shape[0]) for t in tiles)
        for t in tiles:
            if t.ndim != 2 or t.shape[1] != 3:
                raise ValueError(f"each tile must be [N,3] (got {tuple(t.shape)})")
        if any(n == 0 for n in sizes):
            # numpy's min() of an empty array raises in pyntcloud's VoxelGrid.compute
            raise ValueError("zero-size array to reduction operation minimum which has no identity (empty tile)")
        as_t = lambda a: (torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)) if isinstance(a, np.ndarray)
                          else a.to(torch.float64))  # noqa: E731
        pts = torch.cat([as_t(t) for t in tiles]).to(device).contiguous()
        lab = None
        if labels is not None:
            lab = torch.cat([as_t(l).reshape(-1) for l in labels]).to(device).contiguous()
            if lab.numel() != pts.shape[0]:
                raise ValueError("labels and points disagree in length")
        offsets = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int64, device=device)
        return PointBatch(pts, lab, offsets, sizes)


@dataclass
class VoxelGrids:
    counts: Optional[torch.Tensor]       # [B,nz,nx,ny] i32 (None on the occupancy-only path)
    towers: Optional[torch.Tensor]       # [B,nz,nx,ny] i32
    density: Optional[torch.Tensor]      # [B,1,nz,nx,ny] f64  hist_on_voxel
    gt: Optional[torch.Tensor]           # [B,1,nz,nx,ny] f64  reg_on_voxel
    occ: Optional[torch.Tensor]          # [B,1,nz,nx,ny] f32|u8  ToFullDense(density)
    gt_occ: Optional[torch.Tensor]       # [B,1,nz,nx,ny] f32|u8  ToFullDense(gt)
    desc: torch.Tensor                   # [B, 6+nx+ny+nz+3] f64: lo, hi, edges
    dropped: torch.Tensor                # [B] i32
    flags: Optional[torch.Tensor] = None  # [B] i32, occupancy path: tiles redone by the counting kernels
    dims: Optional[torch.Tensor] = None   # [B,3] i32 (n_x, n_y, n_z) per tile -- voxel-size mode: grids are padded to the maximum
    status: Optional[torch.Tensor] = None  # [B] i32, voxel-size mode: 1 = the tile needs more voxels than the maximum
    rider_done: bool = False               # the bank rider handed to voxelize_batch ran with the first launch
    row_bits: Optional[torch.Tensor] = None  # [B,nz,ceil(nx/32)] i32, n-mode occupancy path: which (z, x) rows of occ hold a voxel


def _device_f64(t, name: str, numpy_ok: bool = False) -> torch.Tensor:
    """t as a contiguous f64 tensor on the device it lives on; with numpy_ok a host array is copied to the current one"""
    if numpy_ok and isinstance(t, np.ndarray):
        t = torch.from_numpy(np.ascontiguousarray(t, dtype=np.float64)).to(torch.device("cuda", torch.cuda.current_device()))
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise _hip.HipLibraryError(f"{name} must live on a HIP device; there is no CPU path")
    return t.to(torch.float64).contiguous()


def _labels_list(tower_label) -> List[float]:
    return [float(v) for v in np.array(tower_label).reshape(-1)]


def voxelize_batch(batch: PointBatch, voxelgrid_dims: Sequence[int] = (64, 64, 64),
                   keep_labels: Optional[Sequence[float]] = None, want_density: bool = False,
                   want_gt: bool = False, want_occ: bool = True, want_gt_occ: bool = False,
                   bounds: Optional[torch.Tensor] = None, want_counts: bool = False,
                   occ_dtype: torch.dtype = torch.float32,
                   voxel_dims: Optional[Sequence[float]] = None, bank_rider=None) -> VoxelGrids:
    """voxelize_ply for a whole batch.  `voxelgrid_dims` is (x, y, z) like the reference
    (pcd_processing.py:362-363); grids come back [.., nz, nx, ny] (voxelization.py:193).

    n_x/n_y/n_z mode (voxel_dims None): when only the binary grids are wanted (what SceneNet consumes) and the tile's
    bitmap fits LDS, the occupancy kernels run (LDS atomics, no global atomics); the density / ratio / count outputs
    take the counting kernels.

    Voxel-size mode (`voxel_dims` = (size_x, size_y, size_z), pcd_processing.py:365-367, semKITTI.py:453-455): every
    tile's grid extents follow from its own bounding box, so `voxelgrid_dims` is the MAXIMUM the grids are allocated
    at; each tile's (n_x, n_y, n_z) is computed on the device (no host round trip) and returned in `.dims`, voxels
    beyond a tile's own dims are 0, `.status[b]` = 1 flags a tile that would need more than the maximum."""
    nx, ny, nz = (int(v) for v in voxelgrid_dims)
    want_t = (want_gt or want_gt_occ)
    if want_t and (batch.labels is None or keep_labels is None):
        raise ValueError("ground-truth grids need labels and keep_labels")
    if voxel_dims is not None:
        if bounds is not None:
            raise ValueError("voxel_dims and bounds are mutually exclusive")
        if (want_occ and not (want_density or want_gt or want_counts)
                and _hip.occupancy_supported((nx, ny, nz), 2 if want_gt_occ else 1)):
            # only the binary grids are wanted (what SceneNet consumes; C4's mode): the LDS-bitmap kernels on the padded
            # per-tile tables -- no global atomic per point ([measured] the counting kernels: 1.60 ms per 32 scans of
            # 120 k points at 128^3 against 0.58 ms in n-mode)
            occ, gt_occ, flags, dropped, desc, dims, status, _ = _hip.voxel_occupancy_sized(
                batch.pts, batch.labels if want_t else None, batch.offsets, voxel_dims, (nx, ny, nz),
                _labels_list(keep_labels) if want_t else (), want_gt_occ=want_gt_occ, out_dtype=occ_dtype,
                bank_rider=bank_rider)
            return VoxelGrids(None, None, None, None, occ, gt_occ, desc, dropped, flags, dims, status,
                              rider_done=bank_rider is not None)
        bbox = _hip.voxel_bbox(batch.pts, batch.offsets)
        desc, dims, status = _hip.voxel_desc_sized(bbox, voxel_dims, (nx, ny, nz))
        counts, towers, dropped = _hip.voxel_scatter(batch.pts, batch.labels if want_t else None, batch.offsets, desc,
                                                     (nx, ny, nz), _labels_list(keep_labels) if want_t else (),
                                                     want_towers=want_t)
        density, gt, occ, gt_occ = _hip.voxel_finalize_sized(counts, towers, desc, want_density, want_gt, want_occ,
                                                             want_gt_occ)
        if occ is not None and occ_dtype != torch.float32:
            occ = occ.to(occ_dtype)
        if gt_occ is not None and occ_dtype != torch.float32:
            gt_occ = gt_occ.to(occ_dtype)
        return VoxelGrids(counts, towers, density, gt, occ, gt_occ, desc, dropped, None, dims, status)
    occupancy_only = (want_occ and not (want_density or want_gt or want_counts)
                      and _hip.occupancy_supported((nx, ny, nz), 2 if want_gt_occ else 1))
    if occupancy_only and bounds is None:   # the hot path: bbox, descriptor, bitmap, expansion in four launches
        occ, gt_occ, flags, dropped, desc, _ = _hip.voxel_occupancy_fused(
            batch.pts, batch.labels if want_t else None, batch.offsets, (nx, ny, nz), True,
            _labels_list(keep_labels) if want_t else (), want_gt_occ=want_gt_occ, out_dtype=occ_dtype,
            bank_rider=bank_rider, want_rows=max(nx, ny, nz) <= 64)   # (the grids whose bits the contraction can use)
        grids = VoxelGrids(None, None, None, None, occ, gt_occ, desc, dropped, flags)
        grids.row_bits = _hip.rows_for(occ)
        grids.rider_done = bank_rider is not None
        return grids
    if bounds is None:
        desc, _ = _hip.voxel_prepare(batch.pts, batch.offsets, (nx, ny, nz), regular=True)
    else:
        desc = _hip.voxel_desc(bounds, (nx, ny, nz), from_bounds=True)
    if occupancy_only:
        occ, gt_occ, flags, dropped = _hip.voxel_occupancy(batch.pts, batch.labels if want_t else None,
                                                           batch.offsets, desc, (nx, ny, nz),
                                                           _labels_list(keep_labels) if want_t else (),
                                                           want_gt_occ=want_gt_occ, out_dtype=occ_dtype)
        return VoxelGrids(None, None, None, None, occ, gt_occ, desc, dropped, flags)
    counts, towers, dropped = _hip.voxel_scatter(batch.pts, batch.labels if want_t else None, batch.offsets, desc,
                                                 (nx, ny, nz), _labels_list(keep_labels) if want_t else (),
                                                 want_towers=want_t)
    density, gt, occ, gt_occ = _hip.voxel_finalize(counts, towers, want_density, want_gt, want_occ, want_gt_occ)
    if occ is not None and occ_dtype != torch.float32:
        occ = occ.to(occ_dtype)  # values are exactly 0 / 1
    if gt_occ is not None and occ_dtype != torch.float32:
        gt_occ = gt_occ.to(occ_dtype)
    return VoxelGrids(counts, towers, density, gt, occ, gt_occ, desc, dropped)


def _size_mode_bounds(bbox: np.ndarray, sizes: Sequence[float]):
    """pyntcloud VoxelGrid.compute with size_x/size_y/size_z (pcd_processing.py:365-367): cube the box,
    then extend each axis by ((range // size) + 1) * size - range (range = the ORIGINAL ptp) and set
    n = int((max - min) / size).  Host fp64 arithmetic on the 6 bbox numbers of one tile."""
    xyzmin, xyzmax = bbox[:3].copy(), bbox[3:].copy()
    xyz_range = xyzmax - xyzmin
    margin = max(xyz_range) - xyz_range
    xyzmin = xyzmin - margin / 2
    xyzmax = xyzmax + margin / 2
    n = [1, 1, 1]
    for a, size in enumerate(sizes):
        m = (((xyz_range[a] // size) + 1) * size) - xyz_range[a]
        xyzmin[a] -= m / 2
        xyzmax[a] += m / 2
        n[a] = int((xyzmax[a] - xyzmin[a]) / size)
    return np.concatenate([xyzmin, xyzmax]), tuple(n)


def _voxelize_single(xyz: ArrayLike, labels, tower_label, voxelgrid_dims, voxel_dims, **wants) -> VoxelGrids:
    batch = PointBatch.from_tiles([xyz], None if labels is None else [labels])
    if voxel_dims is None:
        return voxelize_batch(batch, voxelgrid_dims, tower_label, **wants)
    # voxel_dims overrides voxelgrid_dims (torch_transforms.py:74-81); the grid's extents are data dependent.  The whole
    # chain runs on the device with `voxelgrid_dims` as the capacity (sn_voxel_desc_sized: no host round trip in the
    # middle); the tile's own (n_x, n_y, n_z) comes back with the grid, which is then cut to it.  Only a tile that needs
    # MORE than the capacity takes the host route: its bbox decides the allocation.
    cap = tuple(max(int(v), 1) for v in voxelgrid_dims)
    g = voxelize_batch(batch, cap, tower_label, voxel_dims=voxel_dims, **wants)
    meta = torch.cat([g.dims[0], g.status[:1]]).cpu().numpy()   # one small D2H, after everything is enqueued
    n = tuple(int(v) for v in meta[:3])
    if int(meta[3]) == 0:
        cut = lambda t: None if t is None else t[..., :n[2], :n[0], :n[1]].contiguous()   # noqa: E731
        return VoxelGrids(cut(g.counts), cut(g.towers), cut(g.density), cut(g.gt), cut(g.occ), cut(g.gt_occ), g.desc,
                          g.dropped, g.flags, g.dims, g.status)
    bbox = _hip.voxel_bbox(batch.pts, batch.offsets).cpu().numpy()[0]
    bounds, n = _size_mode_bounds(bbox, voxel_dims)
    b = torch.from_numpy(bounds[None]).to(batch.pts.device)
    return voxelize_batch(batch, n, tower_label, bounds=b, **wants)


def hist_on_voxel(xyz, voxelgrid_dims=(64, 64, 64), voxel_dims=None) -> np.ndarray:
    """voxelization.py:164-204: per-voxel point count, min-max normalised per y column -> [nz,nx,ny] f64."""
    g = _voxelize_single(xyz, None, None, voxelgrid_dims, voxel_dims, want_density=True, want_occ=False)
    return g.density[0, 0].cpu().numpy()


def reg_on_voxel(xyz, labels, tower_label, voxelgrid_dims=(64, 64, 64), voxel_dims=None) -> np.ndarray:
    """voxelization.py:244-300: fraction of `tower_label` points per occupied voxel -> [nz,nx,ny] f64."""
    g = _voxelize_single(xyz, labels, tower_label, voxelgrid_dims, voxel_dims, want_gt=True, want_occ=False)
    return g.gt[0, 0].cpu().numpy()


def prob_to_label(voxelgrid, tau: float):
    """voxelization.py:304-323."""
    if isinstance(voxelgrid, torch.Tensor):
        return (voxelgrid >= tau).to(voxelgrid.dtype)
    return (voxelgrid >= tau).astype(voxelgrid.dtype)


def vxg_to_xyz(vxg, origin=None, voxel_size=None, as_tensor: bool = False):
    """voxelization.py:328-360: every cell of the voxel grid as a row (origin + index * voxel_size, value) -> (V, 4)
    f64, rows in C order of the grid's indices.  Returns a numpy array like the reference, or the device tensor with
    `as_tensor`."""
    t = vxg if isinstance(vxg, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(vxg))
    if t.dim() != 3:
        raise ValueError(f"vxg_to_xyz expects a 3-D grid, got shape {tuple(t.shape)}")
    if not t.is_cuda:
        t = t.to(torch.device("cuda", torch.cuda.current_device()))
    if t.dtype not in (torch.float32, torch.float64, torch.uint8, torch.bool):
        t = t.to(torch.float64)
    rows = _hip.grid_to_points(t.contiguous(), origin, voxel_size)
    return rows if as_tensor else rows.cpu().numpy()
