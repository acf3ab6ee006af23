"""The shape of a point's neighbourhood on the device (sn_shape_points, csrc/shape.hip): the covariance of every point's
neighbours within a radius, its eigenvalues, the normal and the principal axis, and the eigenfeatures that tell the classes
of a corridor scan apart -- ground is planar, a conductor linear and horizontal, a tower linear and upright, vegetation
scattered.  The other half of "a point's neighbourhood" next to neighbours.py's distances.

    sh = sna.shape_features(batch, radius=0.9)                # PointShapes: count, moments, eig, normal, axis, feat
    upright = sh.feature("uprightness")
    n = sna.estimate_normals(xyz, radius=0.6, towards=scanner_xyz)
    towers = sna.select_by_shape(batch, 0.9, "uprightness", minimum=0.9)      # ThinnedPoints, as thin_points returns
    sna.write_las(path, xyz, rgb=sna.shape_colors(sh))        # red linear, green planar, blue scattered

Definition (normative, include/scenenet_hip.h): the neighbourhood of row p is p and every row q of its tile with (dx*dx +
dy*dy) + dz*dz <= radius*radius (K21's candidate test; a NaN or infinite coordinate: no neighbours, nobody's neighbour),
with no cap and duplicates included.  Offsets from p are rounded to radius / 65536 and summed as integers, so count and the
nine moments do not depend on the order of the rows or on the grid; covariance, a cyclic Jacobi solver of SN_SHAPE_SWEEPS
sweeps, the ascending sort, the sign rule (n_z >= 0, then n_y >= 0, then n_x > 0) and the features are fp64 operations
rounded once each in the header's order.  A row with fewer than min_points members, or whose members all coincide, has NaN.
This is THIS project's definition: nothing in the reference computes it.
There is no CPU path: CPU tensors raise HipLibraryError.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Sequence, Union

import torch

from . import _hip
from ._hip import SN_SHAPE_NFEAT
from .neighbours import DEFAULT_MAX_CELLS, _as_batch, _tile_grid
from .thin import ThinnedPoints, thin_points
from .voxelization import PointBatch

FEATURE_NAMES = ("linearity", "planarity", "scattering", "surface_variation", "verticality", "uprightness")
assert len(FEATURE_NAMES) == SN_SHAPE_NFEAT
_WANT = ("eig", "normal", "axis", "feat")


@dataclass
class PointShapes:
    """What one shape_features call leaves on the device, indexed by the packed row (scan order).
      count   [total] i32: the members of the row's neighbourhood, the row included; 0 for a row that is not finite
      moments [total, 9] i64 | None: sum f_x, f_y, f_z, then sum f_x f_x, f_x f_y, f_x f_z, f_y f_y, f_y f_z, f_z f_z of the
              members' offsets f = rint((q - p) * 65536 / radius)
      eig     [total, 3] f64 | None: the covariance's eigenvalues ascending, in squared coordinate units
      normal  [total, 3] f64 | None: the unit eigenvector of the smallest, n_z >= 0
      axis    [total, 3] f64 | None: the unit eigenvector of the largest, same sign rule
      feat    [total, 6] f64 | None: FEATURE_NAMES
      offsets [B+1] i64, radius, min_points: the call's own"""
    count: torch.Tensor
    moments: Optional[torch.Tensor]
    eig: Optional[torch.Tensor]
    normal: Optional[torch.Tensor]
    axis: Optional[torch.Tensor]
    feat: Optional[torch.Tensor]
    offsets: torch.Tensor
    radius: float
    min_points: int = 3
    FEATURE_NAMES = FEATURE_NAMES

    def feature(self, name: str) -> torch.Tensor:
        """[total] f64: one column of feat by its name (FEATURE_NAMES)"""
        if name not in FEATURE_NAMES:
            raise ValueError(f"no feature {name!r} (one of {FEATURE_NAMES})")
        if self.feat is None:
            raise ValueError("this call did not ask for feat")
        return self.feat[:, FEATURE_NAMES.index(name)]


def shape_features(batch_or_xyz: Union[PointBatch, torch.Tensor], radius: float, min_points: int = 3,
                   want: Sequence[str] = _WANT, lo=None, extent=None, max_cells: int = DEFAULT_MAX_CELLS,
                   want_moments: bool = True) -> PointShapes:
    """Covariance eigenvalues, normal, principal axis and eigenfeatures of every row's neighbourhood within `radius`, of a
    PointBatch (tiles never see each other) or of xyz [n,3] on the device (one tile); module docstring.
      min_points  rows with fewer members (the row counts) get NaN; at least 3
      want        which of "eig", "normal", "axis", "feat" to compute and return (the others are None)
      lo, extent  lo [B,3] (device tensor) and extent (3 host floats): where each tile's grid starts and how far it reaches.
                  Both given: no synchronisation, capturable.  Otherwise the tiles' boxes come from sn_voxel_bbox with ONE
                  read to the host.  The result is exact for any lo and extent -- they only decide the speed.
      max_cells   the cell budget of the whole batch (at most 2^22)"""
    pts, offsets, _ = _as_batch(batch_or_xyz)
    unknown = [w for w in want if w not in _WANT]
    if unknown:
        raise ValueError(f"want holds {unknown}; it takes {_WANT}")
    min_points = int(min_points)
    if min_points < 3:
        raise ValueError("min_points must be at least 3: a plane needs three points")
    radius = float(radius)
    if not radius > 0.0:
        raise ValueError("radius must be positive")
    dev, total, B = pts.device, int(pts.shape[0]), int(offsets.numel()) - 1
    if total == 0 or B < 1:
        raise ValueError("shape_features needs at least one point")
    lo, dims, mult = _tile_grid(pts, offsets, radius, lo, extent, max_cells)
    ws = torch.empty(_hip.shape_ws_bytes(total, B, dims[0] * dims[1] * dims[2]) // 8, dtype=torch.int64, device=dev)
    new = lambda cols, dtype=torch.float64: torch.empty((total, cols), dtype=dtype, device=dev)   # noqa: E731
    count = torch.empty((total,), dtype=torch.int32, device=dev)
    moments = new(9, torch.int64) if want_moments else None
    eig = new(3) if "eig" in want else None
    normal = new(3) if "normal" in want else None
    axis = new(3) if "axis" in want else None
    feat = new(SN_SHAPE_NFEAT) if "feat" in want else None
    _hip.shape_points(pts, offsets, radius, min_points, lo, dims, mult, ws, count, moments, eig, normal, axis, feat)
    return PointShapes(count, moments, eig, normal, axis, feat, offsets, radius, min_points)


def estimate_normals(xyz: Union[PointBatch, torch.Tensor], radius: float, towards=None, min_points: int = 3,
                     **grid) -> torch.Tensor:
    """[total, 3] f64: the normals of shape_features (n_z >= 0; NaN where a row has fewer than min_points members).
    towards: a viewpoint [3] (tensor or three floats), e.g. the scanner: a normal is negated where n . (towards - p) < 0,
    so that every normal looks at the viewpoint.  The flip is a few torch operations, not a kernel.  `grid`: lo, extent,
    max_cells of shape_features."""
    pts, _, _ = _as_batch(xyz)
    sh = shape_features(xyz, radius, min_points, want=("normal",), want_moments=False, **grid)
    normals = sh.normal
    if towards is not None:
        view = torch.as_tensor(towards, dtype=torch.float64).to(pts.device).reshape(1, 3)
        away = ((view - pts) * normals).sum(dim=1) < 0.0
        normals = torch.where(away[:, None], -normals, normals)
    return normals


def select_by_shape(batch, radius: float, feature: str, minimum: Optional[float] = None, maximum: Optional[float] = None,
                    capacity: Optional[int] = None, labels=None, min_points: int = 3, **grid) -> ThinnedPoints:
    """Keeps the rows whose eigenfeature `feature` (FEATURE_NAMES) is >= minimum, or <= maximum, and returns them as
    thin_points does (scan order, labels, src).  Exactly one of minimum and maximum; a row whose feature is NaN is never
    kept.  Goes through thin_points(u=..., thresholds=[B, 1]) as remove_outliers does -- the rule there is u <= thr;
    `minimum` passes u = -feature, thr = -minimum.  With `capacity` (and lo / extent in `grid`) nothing is read back: the
    chain is capturable.  batch: a PointBatch, or xyz [n,3] with `labels`.
        towers = sna.select_by_shape(batch, 0.9, "uprightness", minimum=0.9)   # upright linear structures"""
    if (minimum is None) == (maximum is None):
        raise ValueError("select_by_shape takes exactly one of minimum and maximum")
    if feature not in FEATURE_NAMES:
        raise ValueError(f"no feature {feature!r} (one of {FEATURE_NAMES})")
    pts, offsets, pb = _as_batch(batch)
    if pb is None:
        lab = None if labels is None else labels.to(torch.float64).reshape(-1).contiguous()
        pb = PointBatch(pts, lab, offsets, (int(pts.shape[0]),))
    elif labels is not None:
        raise ValueError("labels come with the PointBatch")
    B = int(offsets.numel()) - 1
    sh = shape_features(pb, radius, min_points, want=("feat",), want_moments=False, **grid)
    f = sh.feature(feature).contiguous()
    u, bound = (f, float(maximum)) if minimum is None else (-f, -float(minimum))
    thr = torch.full((B, 1), bound, dtype=torch.float64, device=pts.device)
    return thin_points(pb, thresholds=thr, u=u, capacity=capacity)


def shape_colors(shapes: PointShapes) -> torch.Tensor:
    """[total, 3] uint16: rint(65535 * (linearity, planarity, scattering)), 0 where they are NaN -- the classic picture of a
    scan's shapes (red linear, green planar, blue scattered) in the form sna.write_las(rgb=...) takes.  A few torch
    operations, not a kernel."""
    if shapes.feat is None:
        raise ValueError("this PointShapes holds no feat")
    v = torch.round(torch.nan_to_num(shapes.feat[:, :3], nan=0.0).clamp(0.0, 1.0) * 65535.0).to(torch.int32)
    # 0 .. 65535 into the 16 bits of an int16, then read as uint16
    return torch.where(v >= 32768, v - 65536, v).to(torch.int16).view(torch.uint16)
