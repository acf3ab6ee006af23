"""Thinning a point batch on the device: the reference's two downsamplers (sn_thin_count / sn_thin_scatter, csrc/thin.hip).

The reference thins raw points on the host (utils/pcd_processing.py: downsampling :375-420, downsampling_relative_height
:423-474): a Python loop over the points fills a dict of lists keyed by the point's voxel (or z slab) at 64^3, then every
group draws np.random.rand(len(group)) and keeps `group[selected <= threshold]`.  Every point is therefore kept
independently; the voxels decide the threshold (by height) and the ORDER of the result (group by group in order of first
appearance, scan order inside a group).  Here the batch stays in HBM:

    thinned = sna.thin_points(batch, keep=0.5, seed=7)                         # ThinnedPoints: batch, src, unbinned, ...
    thinned = sna.thin_points(batch, keep=0.8, rule="height", seed=7)          # the height rule on K1's z index
    xyz, classes = sna.downsampling_relative_height(xyz, classes, 0.8, seed=7) # the reference's call, its row order

Rule (normative, include/scenenet_hip.h): row j of tile b is kept iff it is binned and u <= thr[b][g], literally (a NaN
keeps nothing); g is 0, K1's z index or K1's flat [z][x][y] index.  u is given, or Philox4x32-10 of (seed; j, tile id) --
`philox_uniforms` restates the generator in numpy.  NOT mirrored: which draw of numpy's global MT19937 stream lands on
which point (the reference hands draws out group by group); the draws are iid, so the result's distribution is the same.
Unpinned, as for K1: pyntcloud's own binning (not installed here); the voxels are K1's, checked against its oracle.
There is no CPU path: CPU tensors raise HipLibraryError.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _hip
from ._hip import SN_THIN_GROUP_NONE, SN_THIN_GROUP_VOXEL, SN_THIN_GROUP_Z, HipLibraryError
from .voxelization import PointBatch, _device_f64

_GROUPS = {"none": SN_THIN_GROUP_NONE, "z": SN_THIN_GROUP_Z, "voxel": SN_THIN_GROUP_VOXEL}
_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_MASK32 = np.uint64(0xFFFFFFFF)


def height_thresholds(sampling_per: float, nz: int) -> np.ndarray:
    """[nz] f64: sampling_per * (1 - z / (nz - 1)) for z = 0 .. nz - 1, the reference's expression operation for operation
    (pcd_processing.py:463-466; z an integer, the division and the rest in fp64).  nz == 1 is 0 / 0: NaN, nothing is kept."""
    z = np.arange(int(nz), dtype=np.int64)
    with np.errstate(divide="ignore", invalid="ignore"):
        normalized_z = z / np.int64(int(nz) - 1)
        return sampling_per * (1 - normalized_z)


def uniform_thresholds(p: float, G: int = 1) -> np.ndarray:
    """[G] f64, all p: every group keeps with the same probability (pcd_processing.py:413)."""
    return np.full((int(G),), float(p), dtype=np.float64)


def philox4x32(counter, key, rounds: int = 10) -> np.ndarray:
    """Philox4x32 (Salmon et al., SC'11): counter [..., 4] and key [..., 2] of 32-bit words -> [..., 4] uint32."""
    c = [np.asarray(counter)[..., i].astype(np.uint64) & _MASK32 for i in range(4)]
    k = [np.asarray(key)[..., i].astype(np.uint64) & _MASK32 for i in range(2)]
    for _ in range(int(rounds)):
        p0, p1 = np.uint64(_M0) * c[0], np.uint64(_M1) * c[2]      # 32 x 32 -> 64 bits: no overflow
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & _MASK32, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & _MASK32]
        k = [(k[0] + np.uint64(_W0)) & _MASK32, (k[1] + np.uint64(_W1)) & _MASK32]
    return np.stack(np.broadcast_arrays(*c), axis=-1).astype(np.uint32)


def philox_uniforms(seed: int, tile_id: int, n: int) -> np.ndarray:
    """[n] f64: what the device draws for rows 0 .. n-1 of the tile `tile_id` under `seed` -- key (seed lo, seed hi),
    counter (j lo, j hi, t lo, t hi), u = ((w0 >> 5) * 2^26 + (w1 >> 6)) * 2^-53: numpy's 53-bit double, in [0, 1)."""
    seed, t = int(seed) & (2 ** 64 - 1), int(tile_id) & (2 ** 64 - 1)
    j = np.arange(int(n), dtype=np.uint64)
    counter = np.stack([j & _MASK32, j >> np.uint64(32), np.full_like(j, t & 0xFFFFFFFF), np.full_like(j, t >> 32)], axis=-1)
    w = philox4x32(counter, np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64)).astype(np.uint64)
    m = ((w[..., 0] >> np.uint64(5)) << np.uint64(26)) | (w[..., 1] >> np.uint64(6))
    return m.astype(np.float64) * 2.0 ** -53


@dataclass
class ThinnedPoints:
    """What one thin_points call leaves on the device.
      batch    PointBatch of the kept rows (offsets: the TRUE sizes; with a capacity, pts / labels have `capacity` rows,
               rows beyond offsets[B] are uninitialised and batch.sizes are the INPUT's sizes, upper bounds)
      src      [rows] int64 | None: each row's index in the packed input
      key      [rows] int32 | None: each row's group (0, z index or flat voxel index)
      unbinned [B] int64: rows of each tile that no table holds (NaN or outside the grid): never kept
      first    [B, G] int64 | None: per group the in-tile index of its first binned row, -1 for an empty group"""
    batch: PointBatch
    src: Optional[torch.Tensor]
    key: Optional[torch.Tensor]
    unbinned: torch.Tensor
    first: Optional[torch.Tensor]


def _seed_tensor(seed, device) -> torch.Tensor:
    """[1] int64 on the device holding the u64's bit pattern."""
    if isinstance(seed, torch.Tensor):
        if not seed.is_cuda or seed.dtype != torch.int64 or seed.numel() != 1:
            raise HipLibraryError("a seed tensor is one int64 on the HIP device")
        return seed
    s = int(seed) & (2 ** 64 - 1)
    return torch.tensor([s - 2 ** 64 if s >= 2 ** 63 else s], dtype=torch.int64, device=device)


def thin_points(batch: Union[PointBatch, torch.Tensor], thresholds=None, keep: Optional[float] = None, rule: str = "uniform",
                group: str = "none", grids=None, voxelgrid_dims: Sequence[int] = (64, 64, 64), seed=None, u=None,
                tile_ids: Optional[torch.Tensor] = None, order: str = "scan", want_src: bool = True, want_key: bool = False,
                labels: Optional[torch.Tensor] = None, capacity: Optional[int] = None) -> ThinnedPoints:
    """Keeps row j of tile b iff u <= thr[b][g] (module docstring) and returns the survivors as a batch.
      batch       a PointBatch, or xyz [n,3] on the device (one tile) with `labels` [n]
      thresholds  [G] or [B, G] (numpy or device tensor), or None: built from `keep` by `rule` -- "uniform": keep for every
                  group; "height": height_thresholds(keep, nz) by the row's z index (group "none" then means "z")
      group       "none" | "z" | "voxel": what g is; the grid is `voxelgrid_dims` (x, y, z) with the descriptor of `grids`
                  (a VoxelGrids or a desc tensor), or sn_voxel_prepare(regular=1) of the batch itself
      seed | u    an int or a [1] int64 device tensor (read by the kernel at run time), or explicit uniforms [total];
                  neither: a seed is drawn from numpy's global generator, as the reference draws from it
      tile_ids    [B] int64 on the device: the tile's id in the counter (default: its index in the batch, or batch.tile_ids)
      order       "scan": stable scan order.  "reference": the kept rows regrouped as the reference returns them -- groups in
                  order of their first appearance in the tile, scan order inside a group.  That is NOT a kernel: a stable
                  torch.sort of the survivors by `first` of their group, on the device.
      capacity    None: count, ONE read of the sizes to the host, exact allocation, scatter.  int: no synchronisation
                  (capturable); whether the rows fit is the caller's to check from batch.offsets[-1].  order "scan" only."""
    if isinstance(batch, PointBatch):
        if labels is not None:
            raise ValueError("labels come with the PointBatch")
        pb = batch
    else:
        pts = _device_f64(batch, "batch", numpy_ok=True)
        if pts.dim() != 2 or pts.shape[1] != 3:
            raise ValueError(f"xyz must be [n, 3] (got {tuple(pts.shape)})")
        n = int(pts.shape[0])
        lab = None if labels is None else _device_f64(labels, "labels", numpy_ok=True).reshape(-1)
        pb = PointBatch(pts, lab, torch.tensor([0, n], dtype=torch.int64, device=pts.device), (n,))
    if not pb.pts.is_cuda:
        raise HipLibraryError("the batch must live on a HIP device; there is no CPU path")
    if rule not in ("uniform", "height") or group not in _GROUPS or order not in ("scan", "reference"):
        raise ValueError(f"unknown rule {rule!r}, group {group!r} or order {order!r}")
    if rule == "height" and group == "none":
        group = "z"
    if order == "reference" and capacity is not None:
        raise ValueError("order='reference' sorts the survivors: it needs their true count (capacity=None)")
    dev = pb.pts.device
    total, B = int(pb.pts.shape[0]), int(pb.offsets.numel()) - 1
    if total == 0:
        raise ValueError("thin_points needs at least one point")
    kind = _GROUPS[group]
    nx, ny, nz = (int(v) for v in voxelgrid_dims)
    G = _hip.thin_groups(kind, (nx, ny, nz))
    desc = None
    if kind != SN_THIN_GROUP_NONE:
        if grids is None:
            desc, _ = _hip.voxel_prepare(pb.pts, pb.offsets, (nx, ny, nz), regular=True)
        else:
            desc = _device_f64(getattr(grids, "desc", grids), "grids", numpy_ok=True)
    if thresholds is None:
        if keep is None:
            raise ValueError("one of thresholds and keep is needed")
        if rule == "height":
            thresholds = height_thresholds(float(keep), nz)
            if kind == SN_THIN_GROUP_VOXEL:
                thresholds = np.repeat(thresholds, nx * ny)       # flat = (iz * nx + ix) * ny + iy
            elif kind == SN_THIN_GROUP_NONE:
                raise ValueError("the height rule needs the z index: group 'z' or 'voxel'")
        else:
            thresholds = uniform_thresholds(float(keep), G)
    thr = _device_f64(thresholds, "thresholds", numpy_ok=True)
    if thr.numel() == G:
        thr = thr.reshape(1, G).expand(B, G).contiguous()
    if tuple(thr.shape) != (B, G):
        raise ValueError(f"thresholds must be [G] or [B, G] = [{B}, {G}] (got {tuple(thr.shape)})")
    if u is not None and seed is not None:
        raise ValueError("u and seed are mutually exclusive")
    if u is not None:
        u = _device_f64(u, "u", numpy_ok=True).reshape(-1)
    else:
        seed = _seed_tensor(np.random.randint(0, 2 ** 63, dtype=np.int64) if seed is None else seed, dev)
    if tile_ids is None:
        tile_ids = getattr(pb, "tile_ids", None)
    if tile_ids is not None:
        tile_ids = tile_ids.to(device=dev, dtype=torch.int64).contiguous()
    reference = order == "reference" and kind != SN_THIN_GROUP_NONE
    want_key_k = want_key or reference

    ws = torch.empty(_hip.thin_ws_bytes(total, B) // 8, dtype=torch.int64, device=dev)
    offsets_out = torch.empty(B + 1, dtype=torch.int64, device=dev)
    unbinned = torch.empty(B, dtype=torch.int64, device=dev)
    first = torch.empty((B, G), dtype=torch.int64, device=dev) if reference else None
    rule_args = (pb.offsets, kind, desc, (nx, ny, nz), thr, u, seed, tile_ids, ws)
    _hip.thin_count(pb.pts, *rule_args, offsets_out, unbinned, first)
    if capacity is None:
        off = offsets_out.cpu().tolist()
        rows, sizes = off[-1], tuple(b - a for a, b in zip(off, off[1:]))
    else:
        rows, sizes = int(capacity), pb.sizes
        if rows < 0:
            raise ValueError("capacity must not be negative")
    out_pts = torch.empty((rows, 3), dtype=torch.float64, device=dev)
    out_labels = torch.empty((rows,), dtype=torch.float64, device=dev) if pb.labels is not None else None
    out_src = torch.empty((rows,), dtype=torch.int64, device=dev) if want_src else None
    out_key = torch.empty((rows,), dtype=torch.int32, device=dev) if want_key_k else None
    if rows > 0:   # (an empty buffer has no address to hand over, and nothing could be written to it)
        _hip.thin_scatter(pb.pts, pb.labels, *rule_args, out_pts, out_labels, out_src, out_key)
    if reference and rows > 0:
        tile = torch.bucketize(torch.arange(rows, device=dev), offsets_out[1:], right=True)
        rank = first[tile, out_key.long()]                  # unique per (tile, group); in-tile indices are < 2^33
        perm = torch.sort(tile * (1 << 34) + rank, stable=True).indices
        out_pts, out_key = out_pts[perm], out_key[perm]
        out_labels = None if out_labels is None else out_labels[perm]
        out_src = None if out_src is None else out_src[perm]
    kept = PointBatch(out_pts, out_labels, offsets_out, sizes, getattr(pb, "tile_ids", None))
    return ThinnedPoints(kept, out_src, out_key if want_key else None, unbinned, first)


def _mirror(xyz, classes, thresholds_of, group: str, seed, u):
    as_numpy = isinstance(xyz, np.ndarray)
    cls_dtype = classes.dtype
    t = thin_points(_device_f64(xyz, "xyz", numpy_ok=True), keep=None, thresholds=thresholds_of(64), group=group, seed=seed,
                    u=u, order="reference", want_src=False, labels=_device_f64(classes, "classes", numpy_ok=True))
    pts, lab = t.batch.pts, t.batch.labels
    if as_numpy:
        return pts.cpu().numpy(), lab.cpu().numpy().astype(cls_dtype)
    return pts, lab.to(cls_dtype)


def downsampling(xyz, classes, samp_per: float = 0.5, seed=None, u=None):
    """pcd_processing.py:375-420 with the array (numpy, or a tensor on the device) in the ply object's place: every point is
    kept iff its uniform <= samp_per; the rows come back voxel by voxel at 64^3 (regular box) in order of each voxel's first
    appearance, scan order inside a voxel -> (xyz [m,3], classes [m]) of the input's kind and class dtype."""
    return _mirror(xyz, classes, lambda nz: uniform_thresholds(samp_per, nz ** 3), "voxel", seed, u)


def downsampling_relative_height(xyz, classes, sampling_per: float = 0.8, seed=None, u=None):
    """pcd_processing.py:423-474: a point of z slab iz (of 64) is kept iff its uniform <= sampling_per * (1 - iz / 63); the
    rows come back slab by slab in order of first appearance -> (xyz [m,3], classes [m]) as downsampling."""
    return _mirror(xyz, classes, lambda nz: height_thresholds(sampling_per, nz), "z", seed, u)


class ThinPoints:
    """A loader transform: ThinPoints(keep, rule, seed)(batch) -> the thinned PointBatch.  The seed lives in a device tensor
    that a torch op advances after every call, so a captured step that holds the call draws anew at every replay (give a
    `capacity` then: no host read); `reseed` rewrites it in place.  A batch that carries `tile_ids` (dataset indices) thins
    a tile the same way wherever it sits in a batch."""

    def __init__(self, keep: float, rule: str = "uniform", seed: int = 0, group: str = "none",
                 voxelgrid_dims: Sequence[int] = (64, 64, 64), capacity: Optional[int] = None, device=None) -> None:
        device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if device.type != "cuda":
            raise HipLibraryError("ThinPoints keeps its seed on a HIP device; there is no CPU path")
        self.keep, self.rule, self.group, self.dims, self.capacity = float(keep), rule, group, tuple(voxelgrid_dims), capacity
        self.seed = _seed_tensor(seed, device)
        nx, ny, nz = (int(v) for v in self.dims)
        kind = _GROUPS["z" if rule == "height" and group == "none" else group]
        thr = height_thresholds(self.keep, nz) if rule == "height" else uniform_thresholds(self.keep, _hip.thin_groups(kind, self.dims))
        if rule == "height" and kind == SN_THIN_GROUP_VOXEL:
            thr = np.repeat(thr, nx * ny)
        self.thresholds = torch.from_numpy(thr).to(device)    # built once: nothing is copied up inside a captured step
        self.last: Optional[ThinnedPoints] = None

    def reseed(self, seed: int) -> None:
        self.seed.copy_(_seed_tensor(seed, self.seed.device))

    def __call__(self, batch: PointBatch) -> PointBatch:
        self.last = thin_points(batch, thresholds=self.thresholds, rule=self.rule, group=self.group, voxelgrid_dims=self.dims,
                                seed=self.seed, capacity=self.capacity)
        self.seed.add_(1)
        return self.last.batch
