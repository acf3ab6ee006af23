"""Accept or reject crop regions on the device: a per-region label census (sn_crop_census, csrc/crops.hip).

The reference decides whether a region of a scan becomes a sample by cutting it, copying it to the host and looking at
its labels there -- utils/pcd_processing.py:742-762 crop_ground_samples (the TS40K no-tower samples),
core/datasets/semKITTI.py:37-88 build_pole_samples, :91-158 crop_tower_samples with build_pole_radius_samples, and the
scan-level gates np.any(classes == TOWER) (ts40k.py:88) / np.any(gt == pole_label) (semKITTI.py:142).  Here the labels
inside all K regions are counted in one pass over the scan in HBM, a few torch operations on K-length tensors give the
acceptance mask on the device, and K9 cuts the accepted regions only (a rejected region gets a kind that is neither disc
nor box: K9 documents it as empty, and it costs nothing in the scatter):

    regions, kinds = sna.slab_regions(starts, width, axis=0, device=dev)
    c = sna.region_census(scan_xyz, regions, kinds, labels=scan_classes, watch=sna.watch_trunc([15]))
    accept = (c.n > 300) & c.distinct_ge2() & (c.watch_counts[:, 0] == 0)          # device, no host read
    crops, accept = sna.crop_accepted(scan_xyz, regions, kinds, scan_classes, accept, capacity=rows)

Definition (normative, include/scenenet_hip.h): membership is K9's, bit for bit (one device function serves both).
n counts the members, n_nan those whose label is NaN, watch_counts[:, c] those with watch[c, 0] <= label <= watch[c, 1]
(inclusive, literal: NaN never matches), label_min / label_max span the members' labels that are not NaN, -0.0 below
+0.0, (+inf, -inf) when there is none.  Everything is an integer sum or a maximum of integer codes: deterministic.
Deviation of the slab mirrors: the reference tests one column (`a[:, idx] >= x`), K9's box test reads both planar
coordinates literally, so a point whose OTHER planar coordinate is NaN is in no slab here.
There is no CPU path: CPU tensors raise HipLibraryError.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _hip
from ._hip import SN_CROP_BOX, SN_CROP_DISC, HipLibraryError
from .crops import ScanCrops, _device_f64, _tower_disc, crop_regions

SN_CROP_REJECTED = -1      # a kinds value that is neither disc nor box: the region is empty


@dataclass
class RegionCensus:
    """What one region_census call leaves on the device, one row per region:
      n, n_nan [K] int64;  label_min, label_max [K] f64 ((+inf, -inf) without a non-NaN label, and without labels);
      watch_counts [K, C] int64;  counts [K, 2 + C] int64 (what the three integer tensors are views of)"""
    n: torch.Tensor
    n_nan: torch.Tensor
    label_min: torch.Tensor
    label_max: torch.Tensor
    watch_counts: torch.Tensor
    counts: torch.Tensor

    def distinct_ge2(self) -> torch.Tensor:
        """bool [K] on the device: len(np.unique(labels of the region)) >= 2, as numpy 2 counts (all NaNs one value, -0.0
        and 0.0 one value).  No host read."""
        return (self.label_min < self.label_max) | ((self.n_nan > 0) & (self.n_nan < self.n))


def _watch_tensor(watch, dev) -> Optional[torch.Tensor]:
    if watch is None:
        return None
    if isinstance(watch, torch.Tensor):
        w = watch.to(device=dev, dtype=torch.float64)
    else:
        w = torch.from_numpy(np.ascontiguousarray(watch, dtype=np.float64)).to(dev)
    w = w.reshape(-1, 2).contiguous()
    return w if w.shape[0] else None


def region_census(pts: torch.Tensor, regions: torch.Tensor, kinds: Optional[torch.Tensor] = None,
                  labels: Optional[torch.Tensor] = None, watch=None) -> RegionCensus:
    """The census of the K regions over the scan pts [n,3] (labels [n] optional; watch [C,2] ranges, a tensor or an array,
    needs labels), module docstring.  One memset node and two launches; nothing is read back."""
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
        raise ValueError("region_census needs at least one point and one region")
    dev = pts.device
    watch = _watch_tensor(watch, dev)
    C = 0 if watch is None else int(watch.shape[0])
    if C and labels is None:
        raise ValueError("watch ranges need labels")
    ws = torch.empty(_hip.crop_census_ws_bytes(n, K, C) // 8, dtype=torch.int64, device=dev)
    counts = torch.empty((K, 2 + C), dtype=torch.int64, device=dev)
    if labels is not None:
        rng = torch.empty((K, 2), dtype=torch.float64, device=dev)
    else:
        rng = None
    _hip.crop_census(pts, labels, regions, kinds, watch, ws, counts, rng)
    if rng is None:
        lo = torch.full((K,), float("inf"), dtype=torch.float64, device=dev)
        hi = torch.full((K,), float("-inf"), dtype=torch.float64, device=dev)
    else:
        lo, hi = rng[:, 0], rng[:, 1]
    return RegionCensus(counts[:, 0], counts[:, 1], lo, hi, counts[:, 2:], counts)


# --------------------------------------------------------------------------- #
def _ranges(rows, device) -> torch.Tensor:
    t = torch.from_numpy(np.array(rows, dtype=np.float64).reshape(-1, 2))
    return t if device is None else t.to(device)


def watch_equal(values: Sequence[float], device=None) -> torch.Tensor:
    """[C,2] f64 ranges (v, v): label == v, what np.isin(labels, values) sums to per value."""
    return _ranges([[float(v), float(v)] for v in values], device)


def watch_trunc(values: Sequence[int], device=None) -> torch.Tensor:
    """[C,2] f64 ranges of the labels l with trunc(l) == v for the integers v -- the reference's `v in labels.astype(int)`
    for the labels astype(int) is defined for: (v, nextafter(v + 1, -inf)) for v > 0, (nextafter(v - 1, +inf), v) for
    v < 0, (nextafter(-1, 0), nextafter(1, 0)) for 0."""
    rows = []
    for v in values:
        if float(v) != int(v):
            raise ValueError(f"watch_trunc takes integers (got {v})")
        v = float(int(v))
        if v > 0:
            rows.append([v, np.nextafter(v + 1.0, -np.inf)])
        elif v < 0:
            rows.append([np.nextafter(v - 1.0, np.inf), v])
        else:
            rows.append([np.nextafter(-1.0, 0.0), np.nextafter(1.0, 0.0)])
    return _ranges(rows, device)


def accept_kinds(kinds: Optional[torch.Tensor], accept: torch.Tensor) -> torch.Tensor:
    """kinds [K] int32 with the rejected regions (accept false) set to SN_CROP_REJECTED, which K9 and the census take as
    an empty region.  kinds None: all discs.  A torch.where on the device."""
    if not isinstance(accept, torch.Tensor) or not accept.is_cuda:
        raise HipLibraryError("accept must live on a HIP device; there is no CPU path")
    accept = accept.reshape(-1).to(torch.bool)
    if kinds is None:
        kinds = torch.full((accept.numel(),), SN_CROP_DISC, dtype=torch.int32, device=accept.device)
    elif not isinstance(kinds, torch.Tensor) or not kinds.is_cuda:
        raise HipLibraryError("kinds must live on a HIP device; there is no CPU path")
    if kinds.numel() != accept.numel():
        raise ValueError("kinds and accept disagree in length")
    return torch.where(accept, kinds.to(torch.int32), torch.full_like(kinds, SN_CROP_REJECTED, dtype=torch.int32))


def crop_accepted(pts: torch.Tensor, regions: torch.Tensor, kinds: Optional[torch.Tensor], labels: Optional[torch.Tensor],
                  accept: Union[torch.Tensor, Callable[[RegionCensus], torch.Tensor]], capacity: Optional[int] = None,
                  watch=None, want_src: bool = True) -> Tuple[ScanCrops, torch.Tensor]:
    """(ScanCrops of the accepted regions -- a rejected region's tile is empty --, accept [K] bool on the device).
    accept: the mask itself, or a predicate that is given the RegionCensus of (pts, regions, kinds, labels, watch) and
    returns it; `watch` goes to that census, so it is refused next to a ready mask (ValueError).  With `capacity` the census, the predicate and K9's two entries run back to back with no synchronisation
    (capturable, as far as the predicate is); without it crop_regions reads offsets[K] once."""
    if not callable(accept) and watch is not None:
        raise ValueError("watch is read by the census behind a predicate; a ready mask takes none")
    if callable(accept):
        accept = accept(region_census(pts, regions, kinds, labels, watch))
    edited = accept_kinds(kinds, accept)
    return crop_regions(pts, regions, edited, labels, capacity=capacity, want_src=want_src), accept.reshape(-1).to(torch.bool)


def slab_regions(starts, width: float, axis: int, device=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(regions [K,4] f64, kinds [K] int32, all boxes) of the slabs start <= coordinate <= start + width: rows
    (x0, -inf, x0 + width, +inf) for axis 0 and (-inf, y0, +inf, y0 + width) for axis 1.  x0 + width is one fp64 addition
    on the host, as in the reference's `a[:, idx] <= x + step`."""
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if device.type != "cuda":
        raise HipLibraryError("slab_regions: the regions live on a HIP device; there is no CPU path")
    if axis not in (0, 1):
        raise ValueError("slab_regions cuts along axis 0 or 1 (the crops are planar)")
    rows = slab_rows(starts, width, axis)
    return torch.from_numpy(rows).to(device), torch.full((rows.shape[0],), SN_CROP_BOX, dtype=torch.int32, device=device)


def slab_rows(starts, width: float, axis: int) -> np.ndarray:
    """The rows of slab_regions as a host array [K, 4]."""
    starts = np.asarray(starts, dtype=np.float64).reshape(-1)
    ends = starts + np.float64(width)
    rows = np.empty((starts.shape[0], 4), dtype=np.float64)
    rows[:, axis], rows[:, 2 + axis] = starts, ends
    rows[:, 1 - axis], rows[:, 3 - axis] = -np.inf, np.inf
    return rows


# --------------------------------------------------------------------------- #
# Mirrors of the reference's label-gated sample builders.  Each returns the accepted samples only, in region order, as
# [n_k, 4] device tensors (x, y, z, class).  Host reads: the scan's extent, which lays out the slabs (the reference's
# np.linspace, on the host; the disc builder reads K10's cluster sizes instead), offsets[K] inside crop_regions for the
# exact allocation, and one read of the offsets together with the acceptance mask, which picks the tiles.
def _accepted_tiles(crops: ScanCrops, accept: torch.Tensor, column=None) -> List[torch.Tensor]:
    """the accepted regions' tiles as [n_k, 4] tensors; ONE host read brings the offsets and the mask"""
    got = torch.cat([crops.offsets, accept.to(torch.int64)]).cpu().tolist()
    K = crops.K
    off, keep = got[:K + 1], got[K + 1:]
    out = []
    for k in range(K):
        if keep[k]:
            p, l = crops.pts[off[k]:off[k + 1]], crops.labels[off[k]:off[k + 1]]
            out.append(torch.cat([p, (l if column is None else column(l))[:, None]], dim=1))
    return out


def _as_int_column(l: torch.Tensor) -> torch.Tensor:
    """`a[:, -1] = a[:, -1].astype(int)` written back into an fp64 column: trunc, and +0.0 for what truncates to zero"""
    return torch.trunc(l) + 0.0


def _slab_starts(lo: float, hi: float, divisor: float) -> Tuple[np.ndarray, int]:
    step = int((hi - lo) / divisor)
    return np.linspace(lo, hi, step), step


def crop_ground_samples(xyz: torch.Tensor, classes: torch.Tensor, max_tower_h: float = 40, tower_class: int = 15
                        ) -> List[torch.Tensor]:
    """pcd_processing.py:742-762 (max_tower_h is not read there either): step = int((xmax - xmin) / 100) slabs
    x0 <= x <= x0 + step from np.linspace(xmin, xmax, step); a slab is a sample iff it holds more than 300 points, at
    least two distinct classes and no class that truncates to tower_class.  The class column comes back truncated, as
    the reference writes astype(int) into it."""
    xyz = _device_f64(xyz, "xyz")
    classes = _device_f64(classes, "classes").reshape(-1)
    lo, hi = torch.stack([xyz[:, 0].min(), xyz[:, 0].max()]).cpu().tolist()
    starts, step = _slab_starts(lo, hi, 100)
    if step == 0:
        return []
    regions, kinds = slab_regions(starts, step, 0, xyz.device)
    crops, accept = crop_accepted(
        xyz, regions, kinds, classes,
        lambda c: (c.n > 300) & c.distinct_ge2() & (c.watch_counts[:, 0] == 0),
        watch=watch_trunc([tower_class]), want_src=False)
    return _accepted_tiles(crops, accept, _as_int_column)


def crop_pole_slabs(xyz: torch.Tensor, gt: torch.Tensor, pole_label: float = 80, min_poles: int = 5, n_steps: int = 10
                    ) -> List[torch.Tensor]:
    """The loop body of semKITTI.py:37-88 build_pole_samples for one scan: slabs along the axis of the largest extent,
    step = int(extent / n_steps), starts np.linspace(min, max, step); a slab is a sample iff at least min_poles of its
    labels equal pole_label.  Labels come back as they are.  Axis 2 is cut from a column-swapped copy of the scan."""
    xyz = _device_f64(xyz, "xyz")
    gt = _device_f64(gt, "gt").reshape(-1)
    ext = torch.stack([xyz.min(dim=0).values, xyz.max(dim=0).values]).cpu().numpy()
    idx = int(np.argmax(ext[1] - ext[0]))
    starts, step = _slab_starts(ext[0][idx], ext[1][idx], n_steps)
    if step == 0:
        return []
    scan = xyz if idx < 2 else xyz[:, [2, 1, 0]].contiguous()
    regions, kinds = slab_regions(starts, step, idx if idx < 2 else 0, xyz.device)
    crops, accept = crop_accepted(scan, regions, kinds, gt, lambda c: c.watch_counts[:, 0] >= int(min_poles),
                                  watch=watch_equal([pole_label]), want_src=False)
    tiles = _accepted_tiles(crops, accept)
    return tiles if idx < 2 else [t[:, [2, 1, 0, 3]] for t in tiles]


def pole_radius_samples(xyz: torch.Tensor, gt: torch.Tensor, pole_label: int = 80, eps: float = 5, min_points: int = 10,
                        radius: float = 5, min_poles: int = 5) -> List[torch.Tensor]:
    """semKITTI.py:91-158 crop_tower_samples under build_pole_radius_samples for one scan: the pole points are clustered
    (cluster_points: DBSCAN(eps, min_points)), one disc of `radius` around each cluster's mean (built as
    crops.crop_tower_samples builds it), and a disc is a sample iff at least min_poles of its classes truncate to
    pole_label -- the reference tests the column crop_tower_radius returned through astype(int), which is also why the
    class column comes back truncated.  A scan without a pole point gives []."""
    from .clusters import cluster_points
    xyz = _device_f64(xyz, "xyz")
    gt = _device_f64(gt, "gt").reshape(-1)
    towers = cluster_points(xyz, eps, min_points, labels=gt, keep=[pole_label]).towers()
    if len(towers) == 0:
        return []
    rows = torch.cat([_tower_disc(t, radius) for t in towers])
    crops, accept = crop_accepted(xyz, rows, None, gt, lambda c: c.watch_counts[:, 0] >= int(min_poles),
                                  watch=watch_trunc([pole_label]), want_src=False)
    return _accepted_tiles(crops, accept, _as_int_column)


def scan_has_class(labels_or_census: Union[torch.Tensor, RegionCensus], value: float = 15, column: int = 0) -> torch.Tensor:
    """The scan-level gate np.any(classes == value) as a 0-dim bool tensor on the device (no host read).  Given labels
    [n]: (labels == value).any(), one torch reduction -- the gate needs no region.  Given a RegionCensus whose watch range
    `column` is (value, value): whether that count is non-zero in any region -- the gate for the part of the scan the
    regions cover, read off a census that was taken anyway (a point in several regions counts in each, which the gate
    does not mind)."""
    if isinstance(labels_or_census, RegionCensus):
        return labels_or_census.watch_counts[:, column].sum() > 0
    labels = _device_f64(labels_or_census, "labels").reshape(-1)
    return (labels == float(value)).any()
