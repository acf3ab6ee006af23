#!/usr/bin/env python3
"""K9 scan crops on a synthetic scan of 10^7 points: 128 tiles of synthetic.py's generator on a 16 x 8 lattice of origins
(a tower in the middle of every tile), concatenated tile after tile.  Regions: K = 8, 32 and 128 discs of r = 15 m at tower
positions, and a lattice of 32 boxes.  Timed between HIP events after a warm-up: sn_crop_count, sn_crop_scatter (labels and
src, exact capacity), and the two captured into a hipGraph and replayed.  Baselines that need none of this library's
kernels: the torch-on-device formulation (per region: mask, nonzero, index_select) and the reference-shaped numpy loop on
the host (np.append of the label column and a[mask] per region, timed on a few regions and scaled), including the copy
of the scan down.  Bytes are the algorithm's: 24 B per point and pass, 8 B label read and 40 B written per output row.
The bench checks what it times: offsets and src against the torch formulation.  Writes one JSON file.
    python tools/crops_bench.py --out profiles/crops_bench.json [--iters 20]"""
import argparse
import gc
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from scene_net_amd import _hip  # noqa: E402
from scene_net_amd.synthetic import synthetic_tile  # noqa: E402

LATTICE, TILE_M = (16, 8), 30.0
HBM_PEAK = 8.0e12      # bytes / s, the part's specification


def timed(fn, iters, spin_ms=100.0):
    """ms per call by events over `iters` calls, after ~100 ms of the same work and a synchronise."""
    gc.collect()
    t0 = time.perf_counter()
    while (time.perf_counter() - t0) * 1e3 < spin_ms:
        fn()
        torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def synthetic_scan(points):
    per_tile = points // (LATTICE[0] * LATTICE[1])
    pts, labels, towers = [], [], []
    for t in range(LATTICE[0] * LATTICE[1]):
        xyz, lab = synthetic_tile(t, per_tile)
        shift = np.array([TILE_M * (t // LATTICE[1]), TILE_M * (t % LATTICE[1]), 0.0])
        pts.append(xyz + shift)
        labels.append(lab)
        towers.append(np.mean(pts[-1][lab == 15.0], axis=0))
    return np.concatenate(pts), np.concatenate(labels), np.array(towers)


def torch_formulation(pts, labels, regions, kinds):
    """per region: mask, nonzero, index_select -- what a user writes without the library; returns (tiles, src)"""
    x, y = pts[:, 0], pts[:, 1]
    out, srcs = [], []
    for row, kind in zip(regions.tolist(), kinds):
        if kind == 0:
            dx, dy = x - row[0], y - row[1]
            mask = torch.add(dx * dx, dy * dy) <= row[2] * row[2]
        else:
            mask = (x >= row[0]) & (x <= row[2]) & (y >= row[1]) & (y <= row[3])
        idx = torch.nonzero(mask).reshape(-1)
        out.append((pts.index_select(0, idx), labels.index_select(0, idx)))
        srcs.append(idx)
    return out, srcs


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
            a[np.sum(np.power((a[:, :-2] - row[:2]), 2), axis=1) <= row[2] * row[2]]
        else:
            a[((row[:2] <= a[:, :2]) & (a[:, :2] <= row[2:4])).all(axis=1)]
    loop = (time.perf_counter() - t0) * len(regions) / timed_regions
    return d2h, loop


def region_case(name, pts, labels, regions_np, kinds_np, iters, host_regions):
    dev = pts.device
    n, K = pts.shape[0], regions_np.shape[0]
    regions = torch.from_numpy(regions_np).to(dev)
    kinds = torch.from_numpy(kinds_np).to(dev)
    ws = torch.empty(_hip.crops_ws_bytes(n, K) // 8, dtype=torch.int64, device=dev)
    offsets = torch.empty(K + 1, dtype=torch.int64, device=dev)
    _hip.crop_count(pts, regions, kinds, ws, offsets)
    total = int(offsets[-1])
    out_pts = torch.empty((total, 3), dtype=torch.float64, device=dev)
    out_lab = torch.empty((total,), dtype=torch.float64, device=dev)
    out_src = torch.empty((total,), dtype=torch.int64, device=dev)

    def count():
        _hip.crop_count(pts, regions, kinds, ws, offsets)

    def scatter():
        _hip.crop_scatter(pts, labels, regions, kinds, ws, offsets, out_pts, out_lab, out_src)

    def both():
        count()
        scatter()
    both()
    want, want_src = torch_formulation(pts, labels, regions, kinds_np.tolist())
    assert offsets.tolist() == [0] + np.cumsum([len(s) for s in want_src]).tolist()
    assert torch.equal(out_src, torch.cat(want_src))
    assert torch.equal(out_pts.view(torch.int64), torch.cat([p for p, _ in want]).view(torch.int64))
    del want, want_src
    t_count, t_scatter, t_both = timed(count, iters), timed(scatter, iters), timed(both, iters)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        both()
    t_replay = timed(graph.replay, iters)
    del graph
    t_torch = timed(lambda: torch_formulation(pts, labels, regions, kinds_np.tolist()), max(2, iters // 4))
    d2h, loop = numpy_loop(pts, labels, regions_np, kinds_np.tolist(), host_regions)
    count_bytes = n * 24 + K * (ws.numel() // K) * 8
    scatter_bytes = n * 24 + total * (8 + 24 + 8 + 8)
    res = {"case": name, "K": K, "rows_out": total,
           "count_us": round(t_count * 1e3, 1), "scatter_us": round(t_scatter * 1e3, 1),
           "count_then_scatter_us": round(t_both * 1e3, 1), "graph_replay_us": round(t_replay * 1e3, 1),
           "count_bytes": count_bytes, "scatter_bytes": scatter_bytes,
           "count_hbm_share": round(count_bytes / (t_count * 1e-3) / HBM_PEAK, 3),
           "scatter_hbm_share": round(scatter_bytes / (t_scatter * 1e-3) / HBM_PEAK, 3),
           "fp64_valu_ops_per_pass": 8 * K * n,
           "torch_formulation_us": round(t_torch * 1e3, 1), "torch_over_replay": round(t_torch / t_replay, 2),
           "host_copy_down_ms": round(d2h * 1e3, 1), "host_numpy_loop_ms": round(loop * 1e3, 1),
           "host_regions_timed": host_regions, "host_over_replay": round((d2h + loop) * 1e3 / t_replay, 1)}
    print(f"{name:18s} K={K:4d} rows {total:9d}  count {res['count_us']:9.1f} us ({res['count_hbm_share']:.2f} of HBM peak)  "
          f"scatter {res['scatter_us']:9.1f} us ({res['scatter_hbm_share']:.2f})  replay {res['graph_replay_us']:9.1f} us  "
          f"torch {res['torch_formulation_us']:10.1f} us  host {res['host_copy_down_ms'] + res['host_numpy_loop_ms']:9.1f} ms",
          flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="crops_bench.json")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--host-regions", type=int, default=2, help="regions the numpy loop runs (scaled to K)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("crops_bench needs a HIP device (there is no CPU path)")
    dev = torch.device("cuda:0")
    xyz, lab, towers = synthetic_scan(args.points)
    pts, labels = torch.from_numpy(xyz).to(dev), torch.from_numpy(lab).to(dev)
    res = {"device": torch.cuda.get_device_name(dev), "points": int(pts.shape[0]), "lattice": list(LATTICE),
           "chunk_points": _hip.crops_chunk_points(), "hbm_peak_bytes_per_s": HBM_PEAK, "cases": []}
    order = np.random.default_rng(0).permutation(len(towers))
    for K in (8, 32, 128):
        rows = np.column_stack([towers[order[:K], :2], np.full(K, 15.0), np.zeros(K)])
        res["cases"].append(region_case("discs r=15 at towers", pts, labels, rows, np.zeros(K, dtype=np.int32), args.iters,
                                        args.host_regions))
    lo, hi = xyz[:, :2].min(axis=0), xyz[:, :2].max(axis=0)
    from scene_net_amd.crops import lattice_boxes
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
