#!/usr/bin/env python3
"""K12 region census on the scan and regions of tools/crops_bench.py: 10^7 points, 32 and 128 discs of r = 15 m at tower
positions, and the lattice of 32 boxes; labels are the scan's classes, one watch range (trunc(label) == 15).  Timed between
HIP events after a warm-up, all in this one run on the same input:
  - sn_crop_census alone (memset node, census, decode);
  - sn_crop_count alone -- the yardstick: the census reads 32 B per point against the count pass's 24 B, so count * 4/3 is
    what an equally efficient census would take; 25 % on top are allowed for the reductions and atomics (a guess at their
    cost, not a measurement);
  - census + predicate (at least 5 tower points) + accept_kinds + sn_crop_count + sn_crop_scatter captured into one hipGraph
    and replayed;
  - a torch formulation on the same device (per region: mask, sum, isin, unique);
  - the reference-shaped numpy loop on the host (np.append, a[mask], len, np.unique, isin; a few regions, scaled), with the
    copy of the scan down.
The bench checks what it times: n, n_nan, the watch count and min / max against the torch formulation.  One JSON file.
    python tools/census_bench.py --out profiles/census_bench.json [--iters 20]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from scene_net_amd import _hip  # noqa: E402
from scene_net_amd.census import RegionCensus, accept_kinds, watch_trunc  # noqa: E402
from scene_net_amd.crops import lattice_boxes  # noqa: E402
from crops_bench import HBM_PEAK, synthetic_scan, timed  # noqa: E402

BYTE_RATIO, MARGIN = 4.0 / 3.0, 1.25
MIN_TOWER_POINTS = 5


def masks(pts, regions, kinds):
    x, y = pts[:, 0], pts[:, 1]
    for row, kind in zip(regions.tolist(), kinds):
        if kind == 0:
            dx, dy = x - row[0], y - row[1]
            yield torch.add(dx * dx, dy * dy) <= row[2] * row[2]
        else:
            yield (x >= row[0]) & (x <= row[2]) & (y >= row[1]) & (y <= row[3])


def torch_formulation(pts, labels, regions, kinds, tower):
    """per region: mask, sum, isin, unique -- what a user writes without the library; [(n, towers, distinct, min, max)]"""
    out = []
    for mask in masks(pts, regions, kinds):
        l = labels[mask]
        u = torch.unique(l)
        out.append((int(mask.sum()), int(torch.isin(torch.trunc(l), tower).sum()), int(u.numel()),
                    float(u[0]) if u.numel() else float("inf"), float(u[-1]) if u.numel() else float("-inf")))
    return out


def numpy_loop(pts_dev, labels_dev, regions, kinds, timed_regions):
    """seconds: the copy down, and the reference-shaped loop over `timed_regions` regions scaled to all of them"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    xyz, classes = pts_dev.cpu().numpy(), labels_dev.cpu().numpy()
    d2h = time.perf_counter() - t0
    t0 = time.perf_counter()
    for row, kind in list(zip(regions, kinds))[:timed_regions]:
        a = np.append(xyz, classes.reshape(-1, 1), axis=1)
        if kind == 0:
            rad = a[np.sum(np.power((a[:, :-2] - row[:2]), 2), axis=1) <= row[2] * row[2]]
        else:
            rad = a[((row[:2] <= a[:, :2]) & (a[:, :2] <= row[2:4])).all(axis=1)]
        _ = len(rad) > 300 and len(np.unique(rad[:, -1])) >= 2 and np.sum(np.isin(rad[:, -1].astype(int), [15])) >= MIN_TOWER_POINTS
    loop = (time.perf_counter() - t0) * len(regions) / timed_regions
    return d2h, loop


def region_case(name, pts, labels, regions_np, kinds_np, iters, host_regions):
    dev = pts.device
    n, K = pts.shape[0], regions_np.shape[0]
    regions = torch.from_numpy(regions_np).to(dev)
    kinds = torch.from_numpy(kinds_np).to(dev)
    watch = watch_trunc([15], device=dev)
    tower = torch.tensor([15.0], dtype=torch.float64, device=dev)
    ws = torch.empty(_hip.crop_census_ws_bytes(n, K, 1) // 8, dtype=torch.int64, device=dev)
    counts = torch.empty((K, 3), dtype=torch.int64, device=dev)
    rng = torch.empty((K, 2), dtype=torch.float64, device=dev)
    cws = torch.empty(_hip.crops_ws_bytes(n, K) // 8, dtype=torch.int64, device=dev)
    offsets = torch.empty(K + 1, dtype=torch.int64, device=dev)

    def census():
        _hip.crop_census(pts, labels, regions, kinds, watch, ws, counts, rng)

    def count():
        _hip.crop_count(pts, regions, kinds, cws, offsets)

    census()
    count()
    total = int(offsets[-1])
    out_pts = torch.empty((total, 3), dtype=torch.float64, device=dev)
    out_lab = torch.empty((total,), dtype=torch.float64, device=dev)
    out_src = torch.empty((total,), dtype=torch.int64, device=dev)
    state = {}

    def sequence():
        census()
        c = RegionCensus(counts[:, 0], counts[:, 1], rng[:, 0], rng[:, 1], counts[:, 2:], counts)
        accept = (c.n > 300) & c.distinct_ge2() & (c.watch_counts[:, 0] >= MIN_TOWER_POINTS)
        edited = accept_kinds(kinds, accept)
        _hip.crop_count(pts, regions, edited, cws, offsets)
        _hip.crop_scatter(pts, labels, regions, edited, cws, offsets, out_pts, out_lab, out_src)
        state["accept"] = accept

    want = torch_formulation(pts, labels, regions, kinds_np.tolist(), tower)
    got_counts, got_rng = counts.cpu().tolist(), rng.cpu().tolist()
    for k, (m, towers, distinct, lo, hi) in enumerate(want):
        assert got_counts[k] == [m, 0, towers] and got_rng[k] == [lo, hi], (k, got_counts[k], got_rng[k], want[k])
    assert torch.equal(counts[:, 0], offsets[1:] - offsets[:-1])
    t_census, t_count = timed(census, iters), timed(count, iters)
    sequence()
    accepted = int(state["accept"].sum())
    rows_accepted = int(offsets[-1])
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        sequence()
    t_replay = timed(graph.replay, iters)
    del graph
    t_torch = timed(lambda: torch_formulation(pts, labels, regions, kinds_np.tolist(), tower), max(2, iters // 4))
    d2h, loop = numpy_loop(pts, labels, regions_np, kinds_np.tolist(), host_regions)
    census_bytes = n * 32 + K * (4 * 8 + 8) + 2 * ws.numel() * 8 + counts.numel() * 8 + rng.numel() * 8
    yardstick = t_count * BYTE_RATIO
    res = {"case": name, "K": K, "C": 1, "census_us": round(t_census * 1e3, 1), "crop_count_us": round(t_count * 1e3, 1),
           "yardstick_us": round(yardstick * 1e3, 1), "census_over_yardstick": round(t_census / yardstick, 3),
           "margin": MARGIN, "within_margin": bool(t_census <= MARGIN * yardstick),
           "census_bytes": census_bytes, "census_bytes_per_s": round(census_bytes / (t_census * 1e-3), 0),
           "census_hbm_share": round(census_bytes / (t_census * 1e-3) / HBM_PEAK, 3),
           "count_hbm_share": round((n * 24 + cws.numel() * 8) / (t_count * 1e-3) / HBM_PEAK, 3),
           "regions_accepted": accepted, "rows_accepted": rows_accepted, "rows_all_regions": total,
           "census_predicate_crop_replay_us": round(t_replay * 1e3, 1),
           "torch_formulation_us": round(t_torch * 1e3, 1), "torch_over_census": round(t_torch / t_census, 1),
           "host_copy_down_ms": round(d2h * 1e3, 1), "host_numpy_loop_ms": round(loop * 1e3, 1),
           "host_regions_timed": host_regions, "host_over_census": round((d2h + loop) * 1e3 / t_census, 1)}
    print(f"{name:18s} K={K:4d}  census {res['census_us']:8.1f} us ({res['census_hbm_share']:.2f} of HBM peak)  count "
          f"{res['crop_count_us']:8.1f} us  census / (count * 4/3) = {res['census_over_yardstick']:.2f}  "
          f"census+predicate+K9 replay {res['census_predicate_crop_replay_us']:9.1f} us ({accepted} accepted)  "
          f"torch {res['torch_formulation_us']:10.1f} us  host {res['host_copy_down_ms'] + res['host_numpy_loop_ms']:9.1f} ms",
          flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="census_bench.json")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--host-regions", type=int, default=2, help="regions the numpy loop runs (scaled to K)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("census_bench needs a HIP device (there is no CPU path)")
    dev = torch.device("cuda:0")
    xyz, lab, towers = synthetic_scan(args.points)
    pts, labels = torch.from_numpy(xyz).to(dev), torch.from_numpy(lab).to(dev)
    res = {"device": torch.cuda.get_device_name(dev), "points": int(pts.shape[0]),
           "chunk_points": _hip.census_chunk_points(), "hbm_peak_bytes_per_s": HBM_PEAK,
           "yardstick": "sn_crop_count in the same run on the same input, times 4/3 for the label bytes; margin 1.25", "cases": []}
    order = np.random.default_rng(0).permutation(len(towers))
    for K in (32, 128):
        rows = np.column_stack([towers[order[:K], :2], np.full(K, 15.0), np.zeros(K)])
        res["cases"].append(region_case("discs r=15 at towers", pts, labels, rows, np.zeros(K, dtype=np.int32), args.iters,
                                        args.host_regions))
    lo, hi = xyz[:, :2].min(axis=0), xyz[:, :2].max(axis=0)
    boxes = lattice_boxes(lo, hi, 60.0, overlap=0.0)
    assert boxes.shape[0] == 32
    res["cases"].append(region_case("box lattice 8 x 4", pts, labels, boxes, np.ones(32, dtype=np.int32), args.iters,
                                    args.host_regions))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
