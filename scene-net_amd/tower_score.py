"""Tower proposals scored against the ground truth on the device (sn_tower_centroids, sn_tower_match, csrc/tower_score.hip).

The reference turns DBSCAN's clusters into its end product on the host, one tile at a time: filter_towers drops walls and
clusters at the rim of the cut-out, aggregate_centroids merges centroids that lie within 1.5 of each other in the plane
(get_tower_proposals, utils/observer_utils.py:476-582), and compute_euc_dists (:413-473) pairs every ground-truth tower
with the nearest proposal and reports their planar distance.  Here all of it reads the [K, 12] statistics rows that
sn_tower_proposals leaves per tile and stays on the device:

    agg = sna.get_tower_proposals(pred, tau=0.65)            # K8, filter (threshold = min_dist / 2), aggregate
    m = sna.compute_euc_dists(pred, gt, tau=0.65)            # K8 on both grids, aggregate, match
    metric = sna.TowerDetectionMetrics(tau=0.65, hit_dist=3.5); metric.update(pred, gt); metric.compute()

The definition is normative in include/scenenet_hip.h (K11): fp64 throughout, every operation rounded once in numpy's
order, so the outputs equal sna.filter_towers / sna.aggregate_centroids and numpy's matching loop bit for bit.  Only
TowerCentroids.rows(b), TowerMatches.sample_distances(b) and TowerDetectionMetrics.compute() synchronise.
There is no CPU path: CPU tensors raise HipLibraryError.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import nn

from . import _hip
from ._hip import HipLibraryError
from .metrics import _ratio, f_beta
from .towers import TowerProposals, tower_proposals

TOTAL_NAMES = ("tiles", "tiles_skipped", "gt_towers", "proposals", "hits", "misses", "false_proposals", "reserved")


class TowerCentroids:
    """What one sn_tower_centroids call leaves on the device, K = the proposals' max_towers:
      keep   [B, K] uint8: 1 for the rows that pass the filter (all present rows without it)
      planar [B, K, 2] fp64: the planar centroid of every present row, NaN rows for absent ones
      agg    [B, K, 2] fp64: the aggregated centroids, sorted as np.unique(axis=0) sorts them; NaN beyond n_agg
      n_agg  [B] int32
      status [B] int32: bit 0 set when the tile had more clusters than K (rows are missing)"""

    def __init__(self, keep, planar, agg, n_agg, status):
        self.keep, self.planar, self.agg, self.n_agg, self.status = keep, planar, agg, n_agg, status

    def rows(self, b: int = 0) -> np.ndarray:
        """aggregate_centroids' return for tile b: [M, 2] fp64 on the host.  Synchronises."""
        m = int(self.n_agg[b])
        return self.agg[b, :m].cpu().numpy()


class TowerMatches:
    """What compute_euc_dists leaves on the device, Kg = max_towers of the ground-truth side:
      centroids   the prediction's TowerCentroids (no filter)
      match       [B, Kg] int32: the index into centroids.agg[b] of the nearest proposal, -1 without one / absent rows
      dist        [B, Kg] fp64: their planar distance; 0.0 when the tile has no proposal; NaN for absent rows
      gt_planar   [B, Kg, 2] fp64: the ground-truth towers' planar centroids, NaN rows for absent ones
      gt_n_towers [B] int32: the ground truth's cluster count, also beyond Kg"""

    def __init__(self, centroids: TowerCentroids, match, dist, gt_planar, gt_n_towers):
        self.centroids, self.match, self.dist, self.gt_planar, self.gt_n_towers = centroids, match, dist, gt_planar, gt_n_towers

    def sample_distances(self, b: int = 0) -> List[Tuple[np.ndarray, Optional[np.ndarray], float]]:
        """The reference's list for tile b: (gt centroid [2], nearest proposal [2] or None, distance) per ground-truth
        tower in id order.  Synchronises."""
        match = self.match[b].cpu().numpy()
        dist = self.dist[b].cpu().numpy()
        g = self.gt_planar[b].cpu().numpy()
        rows = self.centroids.rows(b)
        out = []
        for k in range(match.shape[0]):
            if np.isnan(g[k, 0]):
                continue
            out.append((g[k], rows[match[k]] if match[k] >= 0 else None, float(dist[k])))
        return out


def _scaled_center(props: TowerProposals, center, voxel_size) -> List[float]:
    if center is not None:
        c = [float(v) for v in center]
        if len(c) != 3:
            raise ValueError("center must have 3 entries, one per grid axis")
        return c
    s = [1.0, 1.0, 1.0] if voxel_size is None else [float(v) for v in voxel_size]
    return [float(c) * s[k] for k, c in enumerate(props.grid_center())]


def tower_centroids(props: TowerProposals, threshold: float, center: Optional[Sequence[float]] = None, height_axis: int = 0,
                    tower_height: float = 14.0, radius: float = 15.0, min_euc: float = 1.5,
                    voxel_size: Optional[Sequence[float]] = None, apply_filter: bool = True) -> TowerCentroids:
    """filter_towers, then aggregate_centroids, over the statistics rows of `props` (module docstring).  threshold,
    tower_height, radius and min_euc are in the units of voxel_size (default 1, 1, 1: index units, like `props`); center: the
    filter's centre in those units (default: props.grid_center() * voxel_size).  apply_filter=False keeps every cluster
    (compute_euc_dists' form).  One launch on the current stream, no synchronisation: capturable."""
    if not isinstance(props.stats, torch.Tensor) or not props.stats.is_cuda:
        raise HipLibraryError("tower_centroids: the proposals must live on a HIP device; there is no CPU path")
    if height_axis not in (0, 1, 2):
        raise ValueError("height_axis must be 0, 1 or 2")
    stats, n_towers = props.stats.contiguous(), props.n_towers.contiguous()
    B, K = int(stats.shape[0]), int(stats.shape[1])
    dev = stats.device
    threshold, radius = float(threshold), float(radius)
    rim_sq = (radius - threshold * 2) ** 2          # evaluated as filter_towers evaluates it, never in the kernel
    ctr = _scaled_center(props, center, voxel_size) if apply_filter else None
    keep = torch.empty((B, K), dtype=torch.uint8, device=dev)
    planar = torch.empty((B, K, 2), dtype=torch.float64, device=dev)
    agg = torch.empty((B, K, 2), dtype=torch.float64, device=dev)
    n_agg = torch.empty((B,), dtype=torch.int32, device=dev)
    status = torch.empty((B,), dtype=torch.int32, device=dev)
    _hip.tower_centroids(stats, n_towers, height_axis, ctr, apply_filter, threshold, float(tower_height), rim_sq,
                         float(min_euc), keep, planar, agg, n_agg, status, voxel_size=voxel_size)
    return TowerCentroids(keep, planar, agg, n_agg, status)


def get_tower_proposals(pred: torch.Tensor, tau: Optional[float] = None, min_dist: float = 3.5, min_points: int = 18,
                        max_towers: int = 64, **filter_kw) -> TowerCentroids:
    """The reference's chain (utils/observer_utils.py:556-582): DBSCAN(eps=min_dist, min_points) over pred >= tau, the
    wall / rim filter with threshold = min_dist / 2, the aggregation.  filter_kw: tower_centroids' keywords (center,
    height_axis, tower_height, radius, min_euc, voxel_size).  Its "remove buggy centroid" step is not mirrored: a centroid
    of exactly (0, 0, 0) needs a cluster of the single voxel (0, 0, 0), which no min_points >= 2 produces."""
    props = tower_proposals(pred, tau, eps=min_dist, min_points=min_points, voxel_size=filter_kw.get("voxel_size"),
                            max_towers=max_towers)
    return tower_centroids(props, float(min_dist) / 2, **filter_kw)


def _match(cents: TowerCentroids, gt_props: TowerProposals, height_axis, voxel_size, hit_dist, totals=None,
           dist_total=None) -> TowerMatches:
    stats = gt_props.stats.contiguous()
    B, Kg = int(stats.shape[0]), int(stats.shape[1])
    dev = stats.device
    match = torch.empty((B, Kg), dtype=torch.int32, device=dev)
    dist = torch.empty((B, Kg), dtype=torch.float64, device=dev)
    gt_planar = torch.empty((B, Kg, 2), dtype=torch.float64, device=dev)
    _hip.tower_match(cents.agg, cents.n_agg, cents.status, stats, gt_props.n_towers.contiguous(), height_axis, hit_dist,
                     match, dist, gt_planar, totals, dist_total, voxel_size=voxel_size)
    return TowerMatches(cents, match, dist, gt_planar, gt_props.n_towers)


def compute_euc_dists(pred: torch.Tensor, gt: torch.Tensor, tau: Optional[float] = None, min_dist: float = 3.5,
                      min_points: int = 18, max_towers: int = 64, hit_dist: float = math.inf, height_axis: int = 0,
                      min_euc: float = 1.5, voxel_size: Optional[Sequence[float]] = None) -> TowerMatches:
    """utils/observer_utils.py:413-473: DBSCAN(eps=min_dist, min_points) on the prediction and on the ground truth, the
    prediction's centroids aggregated (no filter), and for every ground-truth tower the nearest aggregated centroid and
    their planar distance.  gt: a bool / uint8 grid (non-zero is tower) or a float grid thresholded at the same tau, as
    tower_proposals takes it.  hit_dist is validated and otherwise unused: no totals are kept here (TowerDetectionMetrics).
    No synchronisation."""
    props = tower_proposals(pred, tau, eps=min_dist, min_points=min_points, voxel_size=voxel_size, max_towers=max_towers)
    gt_props = tower_proposals(gt, tau, eps=min_dist, min_points=min_points, voxel_size=voxel_size, max_towers=max_towers)
    if gt_props.stats.shape[0] != props.stats.shape[0]:
        raise ValueError(f"pred has {props.stats.shape[0]} tiles, gt {gt_props.stats.shape[0]}")
    cents = tower_centroids(props, float(min_dist) / 2, height_axis=height_axis, min_euc=min_euc, voxel_size=voxel_size,
                            apply_filter=False)
    return _match(cents, gt_props, height_axis, voxel_size, float(hit_dist))


def tower_detection_values(totals: Sequence[int], dist_total: float) -> Dict[str, float]:
    """The metric's values from the accumulated totals (TOTAL_NAMES) in fp64, 0/0 -> 0: recall = hits / gt_towers,
    precision = (proposals - false_proposals) / proposals, f1, mean_error = dist_total / hits; plus the raw counts."""
    t = dict(zip(TOTAL_NAMES, (int(v) for v in totals)))
    recall = _ratio(float(t["hits"]), float(t["gt_towers"]))
    precision = _ratio(float(t["proposals"] - t["false_proposals"]), float(t["proposals"]))
    out: Dict[str, float] = {"recall": recall, "precision": precision, "f1": f_beta(precision, recall, 1.0),
                             "mean_error": _ratio(float(dist_total), float(t["hits"]))}
    out.update({k: v for k, v in t.items() if k != "reserved"})
    out["dist_total"] = float(dist_total)
    return out


class TowerDetectionMetrics(nn.Module):
    """Tower-level detection quality, accumulated on the device: every update runs DBSCAN(eps, min_points) on pred >= tau
    and on gt, filters (apply_filter; threshold defaults to eps / 2 as get_tower_proposals sets it) and aggregates the
    prediction's clusters, pairs every ground-truth tower with its nearest proposal and adds the tile's counts to `totals`
    (TOTAL_NAMES) and the hits' distances to `dist_total`.  A ground-truth tower is a hit when its nearest proposal lies
    within hit_dist; hit_dist defaults to eps (pass it to choose another radius; math.inf counts every pairing).  Tiles with
    more clusters than max_towers on either side count as tiles_skipped only.

    update(pred, gt): no synchronisation, no host copy, capturable.  compute() (one synchronisation) returns Python
    floats / ints: recall, precision, f1, mean_error in fp64 with 0/0 -> 0, and the raw counts.  reset() zeroes the state.
    The state moves with .to(device) and adds no state-dict keys."""

    def __init__(self, tau: float = 0.65, eps: float = 3.5, min_points: int = 18, hit_dist: Optional[float] = None,
                 apply_filter: bool = True, max_towers: int = 64, threshold: Optional[float] = None,
                 center: Optional[Sequence[float]] = None, height_axis: int = 0, tower_height: float = 14.0,
                 radius: float = 15.0, min_euc: float = 1.5, voxel_size: Optional[Sequence[float]] = None):
        super().__init__()
        if not 0.0 < float(tau) < 1.0:
            raise ValueError(f"tau must lie in (0, 1) (got {tau})")
        self.tau, self.eps, self.min_points, self.max_towers = float(tau), float(eps), int(min_points), int(max_towers)
        self.hit_dist = self.eps if hit_dist is None else float(hit_dist)
        if not self.hit_dist > 0.0:
            raise ValueError(f"hit_dist must be positive (got {hit_dist})")
        self.apply_filter = bool(apply_filter)
        self.threshold = self.eps / 2 if threshold is None else float(threshold)
        self.center = None if center is None else [float(v) for v in center]
        self.height_axis, self.tower_height, self.radius, self.min_euc = int(height_axis), float(tower_height), \
            float(radius), float(min_euc)
        self.voxel_size = None if voxel_size is None else [float(v) for v in voxel_size]
        self.register_buffer("totals", torch.zeros(_hip.SN_TSCORE_NTOTAL, dtype=torch.int64), persistent=False)
        self.register_buffer("dist_total", torch.zeros(1, dtype=torch.float64), persistent=False)

    @torch.no_grad()
    def update(self, pred: torch.Tensor, gt: torch.Tensor) -> TowerMatches:
        if not isinstance(pred, torch.Tensor) or not pred.is_cuda or not isinstance(gt, torch.Tensor) or not gt.is_cuda:
            raise HipLibraryError("TowerDetectionMetrics: pred and gt must live on a HIP device; there is no CPU path")
        if self.totals.device != pred.device:
            raise HipLibraryError(f"the metric's state lives on {self.totals.device}: move the module with "
                                  f".to({pred.device}) first")
        props = tower_proposals(pred, self.tau, eps=self.eps, min_points=self.min_points, voxel_size=self.voxel_size,
                                max_towers=self.max_towers)
        gt_props = tower_proposals(gt, self.tau, eps=self.eps, min_points=self.min_points, voxel_size=self.voxel_size,
                                   max_towers=self.max_towers)
        if gt_props.stats.shape[0] != props.stats.shape[0]:
            raise ValueError(f"pred has {props.stats.shape[0]} tiles, gt {gt_props.stats.shape[0]}")
        cents = tower_centroids(props, self.threshold, center=self.center, height_axis=self.height_axis,
                                tower_height=self.tower_height, radius=self.radius, min_euc=self.min_euc,
                                voxel_size=self.voxel_size, apply_filter=self.apply_filter)
        return _match(cents, gt_props, self.height_axis, self.voxel_size, self.hit_dist, self.totals, self.dist_total)

    def forward(self, pred: torch.Tensor, gt: torch.Tensor) -> TowerMatches:
        return self.update(pred, gt)

    def compute(self) -> Dict[str, float]:
        return tower_detection_values(self.totals.tolist(), float(self.dist_total.item()))

    def reset(self) -> None:
        self.totals.zero_()
        self.dist_total.zero_()

    def extra_repr(self) -> str:
        return (f"tau={self.tau}, eps={self.eps}, min_points={self.min_points}, hit_dist={self.hit_dist}, "
                f"apply_filter={self.apply_filter}, max_towers={self.max_towers}")
