"""Tile predictions put back on the whole scan in one pass (K19: sn_scan_merge, csrc/scan_merge.hip), and the product flow on
top of it: "a corridor scan in, tower probabilities per scan point out".

    seg = sna.segment_scan(model, scan_xyz)                          # lattice -> crops -> pipeline -> one merge
    seg.prob [C, n], seg.cover [n]
    sna.classify_las("in.las", "out.las", model, tau=0.5)            # the same, file to file

The long form, for a caller who keeps the pieces:

    regions, kinds = sna.lattice_regions(lo_xy, hi_xy, tile=30.0, overlap=5.0)
    crops = sna.crop_regions(scan_xyz, regions, kinds, want_src=False)
    batch, kept = crops.point_batch()                                # empty tiles dropped
    out, grids = ...                                                 # the model over the batch, and its voxelisation
    prob = sna.scan_predictions(out, scan_xyz, regions, kinds, grids, kept, rule="interior")

Definition (normative, include/scenenet_hip.h): region k COVERS scan point i iff it has a tile, the point is a member of k
by K9's test (crops.py) and the point bins inside that tile's edge table by sn_gather_points' rule.  `cover` counts the
covering regions; a point with none reads `fill`.  rule "max": the largest covering value (NaN if one is NaN); "mean": the
fp64 sum in region order over the count; "interior": the value of the region the point lies deepest in, ties to the lowest
index -- depth is measured in the REGION's geometry (distance to the box's nearest side, r - distance to the disc's
centre), not in the grid's, which is built from the members' bounding cube.  With overlapping tiles "interior" is the rule
for this model: its convolutions pad with zeros, so a tile's prediction is least reliable at its faces, and "max" picks
that artefact whenever it is the larger value.
The difference to merge_to_scan(point_predictions(...)): a member that bins outside its tile's table is not covered by that
tile; there it competed with the value `fill`.  There is no CPU path: CPU tensors raise HipLibraryError.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _hip
from ._hip import HipLibraryError
from .crops import crop_regions, lattice_regions
from .pipeline import ScenePipeline
from .voxelization import PointBatch, VoxelGrids

RULES = {"max": _hip.SN_MERGE_MAX, "mean": _hip.SN_MERGE_MEAN, "interior": _hip.SN_MERGE_INTERIOR}


def tile_of_kept(kept: Sequence[int], K: int) -> np.ndarray:
    """[K] int32: the tile of every region, given the regions a batch holds in its order (what ScanCrops.point_batch()
    returns); a region not in `kept` gets -1 (no tile: covers nothing).  Host arithmetic."""
    kept = [int(k) for k in kept]
    if any(k < 0 or k >= K for k in kept):
        raise ValueError(f"kept names a region outside 0..{K - 1}")
    if len(set(kept)) != len(kept):
        raise ValueError("kept names a region twice")
    tile_of = np.full(int(K), -1, dtype=np.int32)
    tile_of[kept] = np.arange(len(kept), dtype=np.int32)
    return tile_of


def _on_device(t, name: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise HipLibraryError(f"{name} must live on a HIP device; there is no CPU path")
    return t


def scan_predictions(pred: torch.Tensor, scan_pts: torch.Tensor, regions: torch.Tensor, kinds: Optional[torch.Tensor],
                     grids_or_desc, kept: Optional[Sequence[int]] = None, rule: str = "max", fill: float = 0.0,
                     want_cover: bool = False):
    """pred [B,C,nz,nx,ny] (f32|f64), the prediction of B tiles, -> [C, n] on the scan scan_pts [n,3] the K regions were cut
    from (and cover [n] int32 with want_cover).  grids_or_desc: the VoxelGrids of the batch, or its desc [B, desc_len].
    kept: the regions the B tiles belong to, in the batch's order (ScanCrops.point_batch()); None: tile k is region k and
    B == K.  One launch; nothing is read back, nothing synchronises."""
    if rule not in RULES:
        raise ValueError(f"rule must be one of {sorted(RULES)} (got {rule!r})")
    desc = grids_or_desc.desc if isinstance(grids_or_desc, VoxelGrids) else grids_or_desc
    pred, desc = _on_device(pred, "pred"), _on_device(desc, "desc")
    scan_pts, regions = _on_device(scan_pts, "scan_pts"), _on_device(regions, "regions")
    if kinds is not None:
        kinds = _on_device(kinds, "kinds").to(torch.int32).contiguous()
    if pred.dim() != 5:
        raise ValueError(f"pred must be [B, C, nz, nx, ny] (got {tuple(pred.shape)})")
    scan_pts = scan_pts.to(torch.float64).contiguous()
    regions = regions.to(torch.float64).contiguous()
    if scan_pts.dim() != 2 or scan_pts.shape[1] != 3 or scan_pts.shape[0] == 0:
        raise ValueError(f"scan_pts must be [n, 3] with n >= 1 (got {tuple(scan_pts.shape)})")
    B, C = int(pred.shape[0]), int(pred.shape[1])
    n, K = int(scan_pts.shape[0]), int(regions.shape[0])
    dev = pred.device
    tile_of = None
    if kept is not None:
        if len(kept) != B:
            raise ValueError(f"kept names {len(kept)} regions for a prediction of {B} tiles")
        tile_of = torch.from_numpy(tile_of_kept(kept, K)).to(dev)
    elif B != K:
        raise ValueError(f"without kept tile k is region k: the prediction holds {B} tiles for {K} regions")
    out = torch.empty((C, n), dtype=pred.dtype, device=dev)
    cover = torch.empty((n,), dtype=torch.int32, device=dev) if want_cover else None
    _hip.scan_merge(pred.contiguous(), desc.contiguous(), scan_pts, regions, kinds, tile_of, RULES[rule], fill, out, cover)
    return (out, cover) if want_cover else out


@dataclass
class ScanSegmentation:
    """What segment_scan leaves on the device: prob [C, n] (the model's output per scan point), cover [n] int32 (tiles that
    cover the point; 0: prob is `fill`), regions [K,4] f64, kinds [K] int32 | None, and kept: the regions that held a
    point, in the order their tiles were predicted."""
    prob: torch.Tensor
    cover: torch.Tensor
    regions: torch.Tensor
    kinds: Optional[torch.Tensor]
    kept: List[int]


class _GridPipeline(ScenePipeline):
    """ScenePipeline whose call hands back the voxelisation next to the prediction: the merge needs its descriptor."""

    def _finish(self, out, grids, batch, want_gt):
        return out, grids


def tile_groups(n_tiles: int, batch_tiles: int) -> List[range]:
    """The tiles of each pipeline call: consecutive groups of at most batch_tiles.  Host arithmetic."""
    if int(batch_tiles) < 1:
        raise ValueError("batch_tiles must be at least 1")
    return [range(a, min(a + int(batch_tiles), int(n_tiles))) for a in range(0, int(n_tiles), int(batch_tiles))]


def group_batch(batch: PointBatch, tiles: range, starts: Sequence[int]) -> PointBatch:
    """Tiles `tiles` of the batch as a batch of their own: the rows are a view, the offsets start at 0 again.  starts: the
    batch's offsets on the host."""
    a, b = tiles.start, tiles.stop
    lo, hi = int(starts[a]), int(starts[b])
    offsets = batch.offsets[a:b + 1] - lo
    return PointBatch(batch.pts[lo:hi], None if batch.labels is None else batch.labels[lo:hi], offsets, batch.sizes[a:b])


def segment_scan(model, scan_pts: torch.Tensor, regions: Optional[torch.Tensor] = None, kinds: Optional[torch.Tensor] = None,
                 *, tile: float = 30.0, overlap: float = 5.0, grid: Sequence[int] = (64, 64, 64), rule: str = "interior",
                 batch_tiles: int = 32, fill: float = 0.0, **pipeline_kw) -> ScanSegmentation:
    """The model over a whole scan scan_pts [n,3]: regions (None: lattice_regions of `tile` and `overlap` over the scan's
    xy box, which is computed on the device; the scan's x and y must then be finite) -> crop_regions(want_src=False) ->
    ScenePipeline(model, grid, **pipeline_kw) over groups of at most batch_tiles tiles, every group's prediction and
    descriptor kept in one resident [K', C, nz, nx, ny] / [K', desc_len] pair -> ONE scan_predictions with `rule`.
    Runs under torch.no_grad().  Synchronises (the crops' sizes come to the host)."""
    scan_pts = _on_device(scan_pts, "scan_pts").to(torch.float64).contiguous()
    if scan_pts.dim() != 2 or scan_pts.shape[1] != 3 or scan_pts.shape[0] == 0:
        raise ValueError(f"scan_pts must be [n, 3] with n >= 1 (got {tuple(scan_pts.shape)})")
    if rule not in RULES:
        raise ValueError(f"rule must be one of {sorted(RULES)} (got {rule!r})")
    dev = scan_pts.device
    with torch.no_grad():
        if regions is None:
            if kinds is not None:
                raise ValueError("kinds without regions")
            box = torch.cat([scan_pts[:, :2].min(dim=0).values, scan_pts[:, :2].max(dim=0).values]).cpu().numpy()
            regions, kinds = lattice_regions(box[:2], box[2:], tile, overlap, device=dev)
        else:
            regions = _on_device(regions, "regions").to(torch.float64).contiguous()
            if kinds is not None:
                kinds = _on_device(kinds, "kinds").to(torch.int32).contiguous()
        crops = crop_regions(scan_pts, regions, kinds, want_src=False)
        batch, kept = crops.point_batch()
        pipe = _GridPipeline(model, tuple(int(v) for v in grid), per_point=False, **pipeline_kw)
        groups = tile_groups(len(kept), batch_tiles)
        starts = np.concatenate([[0], np.cumsum(batch.sizes)])
        pred = desc = None
        for tiles in groups:
            out, grids = pipe(batch if len(groups) == 1 else group_batch(batch, tiles, starts))
            if out.dtype not in (torch.float32, torch.float64):
                out = out.float()
            if len(groups) == 1:
                pred, desc = out, grids.desc
                break
            if pred is None:
                pred = torch.empty((len(kept),) + tuple(out.shape[1:]), dtype=out.dtype, device=dev)
                desc = torch.empty((len(kept), grids.desc.shape[1]), dtype=torch.float64, device=dev)
            pred[tiles.start:tiles.stop].copy_(out)
            desc[tiles.start:tiles.stop].copy_(grids.desc)
        prob, cover = scan_predictions(pred, scan_pts, regions, kinds, desc, kept, rule, fill, want_cover=True)
    return ScanSegmentation(prob, cover, regions, kinds, kept)


def classify_las(src: str, dst: str, model, tau: float, tower_class: int = 15, **segment_kw) -> ScanSegmentation:
    """LAS in, classified LAS out: read_las(src) -> segment_scan(model, xyz, **segment_kw) -> every point whose channel-0
    probability is >= tau becomes `tower_class`, the others keep their class -> reclassify_las(src, dst, classes), which
    keeps every other byte of the file.  Returns the ScanSegmentation."""
    from .las import read_las
    from .las_write import reclassify_las
    dev = next(model.parameters()).device
    if dev.type != "cuda":
        raise HipLibraryError("classify_las: the model must live on a HIP device; there is no CPU path")
    scan = read_las(src, device=dev, want_hist=False)
    seg = segment_scan(model, scan.xyz, **segment_kw)
    classes = torch.where(seg.prob[0] >= tau, torch.full_like(scan.classes, float(tower_class)), scan.classes)
    reclassify_las(src, dst, classes)
    return seg
