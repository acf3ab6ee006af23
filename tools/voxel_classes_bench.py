#!/usr/bin/env python3
"""K18 on the C2 batch (32 tiles of 10^5 points, 64^3) and on the classes of one synthetic scan of 10^7 points.  Timed
between HIP events after a warm-up, eager and captured into a hipGraph and replayed.
Grid: sn_voxel_classes with and without the skip-if-not-larger load.  Yardstick, measured in the same run: sn_voxel_scatter
with tower counts + sn_voxel_finalize with `gt` on the same batch -- the same 32 B read per point, two 32-bit atomics per
point where K18 makes one 64-bit one, the same bytes of grid written.  The mark is that time plus 25 %.
Colours: sn_class_census + sn_class_paint in the `colors` (f64) and the `rgb` (u16) form.  Yardstick, measured in the same
run: a device copy_ that moves the same total bytes (8 B read in the census, 8 B read and 24 or 6 B written in the paint:
40 or 22 B per row, so a copy of 20 or 11 B per row).  The mark is that time plus 25 %.
Baselines that need none of this library's kernels: the torch formulation on the device (searchsorted + scatter_reduce(amax)
for the grid; unique / searchsorted / index_select for the colours) and the reference-shaped host code (the pandas groupby
and loop; the per-point colour loop), timed on 10^5 points and SCALED linearly to the input's size.
The bench checks what it times against the torch formulation, bit for bit.  Writes one JSON file.
    python tools/voxel_classes_bench.py --out profiles/voxel_classes_bench.json [--iters 20]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from crops_bench import HBM_PEAK, synthetic_scan, timed  # noqa: E402
from scene_net_amd import _hip  # noqa: E402
from scene_net_amd.synthetic import synthetic_tile  # noqa: E402

DIMS = (64, 64, 64)
ALLOWANCE = 1.25


def replayed(fn, iters):
    fn()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fn()
    t = timed(graph.replay, iters)
    del graph
    return t


def both_ways(fn, iters):
    return {"eager_us": round(timed(fn, iters) * 1e3, 1), "graph_replay_us": round(replayed(fn, iters) * 1e3, 1)}


def verdict(mine, yard):
    mark = round(yard["graph_replay_us"] * ALLOWANCE, 1)
    return {"graph_replay_us": mine["graph_replay_us"], "yardstick_graph_replay_us": yard["graph_replay_us"], "mark_us": mark,
            "over_yardstick": round(mine["graph_replay_us"] / yard["graph_replay_us"], 3),
            "position": "INSIDE" if mine["graph_replay_us"] <= mark else "OUTSIDE"}


# ---------------------------------------------------------------- the class grid
def flat_index_torch(pts, offsets, desc):
    """[total] int64: b * V + the flat [z][x][y] index by searchsorted on the tile's edge tables (own points: all inside)"""
    nx, ny, nz = DIMS
    B = offsets.numel() - 1
    sizes = (offsets[1:] - offsets[:-1])
    tile = torch.repeat_interleave(torch.arange(B, device=pts.device), sizes)
    idx = []
    start = 6
    for a, n in enumerate(DIMS):
        edges = desc[:, start:start + n + 1].contiguous()
        start += n + 1
        # (a ragged batch against one table per tile: tile by tile)
        k = torch.empty_like(tile)
        for b in range(B):
            sl = slice(int(offsets[b]), int(offsets[b + 1]))
            k[sl] = torch.searchsorted(edges[b], pts[sl, a].contiguous(), right=False) - 1
        idx.append(k.clamp_(0, n - 1))
    return tile * (nx * ny * nz) + (idx[2] * nx + idx[0]) * ny + idx[1]


def grid_host_loop(xyz, labels, desc_row):
    """seconds of the reference's DataFrame, groupby.max and loop (voxelization.py:232-239), voxel indices given"""
    import pandas as pd
    nx, ny, nz = DIMS
    e = [desc_row[6:6 + nx + 1], desc_row[6 + nx + 1:6 + nx + ny + 2], desc_row[6 + nx + ny + 2:]]
    vx, vy, vz = (np.clip(np.searchsorted(e[a], xyz[:, a], side="left") - 1, 0, DIMS[a] - 1) for a in range(3))
    t0 = time.perf_counter()
    data = np.zeros((nz, nx, ny))
    voxs = pd.DataFrame({"label": labels, "z": vz, "x": vx, "y": vy})
    groups = voxs.groupby(["z", "x", "y"]).max()
    for i, hist in groups.iterrows():
        data[i] = hist.iloc[0]
    return time.perf_counter() - t0


def grid_case(args):
    dev = torch.device("cuda:0")
    nx, ny, nz = DIMS
    tiles, labels = zip(*[synthetic_tile(t, args.tile_points) for t in range(args.batch)])
    sizes = [len(t) for t in tiles]
    pts = torch.from_numpy(np.concatenate(tiles)).to(dev)
    lab = torch.from_numpy(np.concatenate(labels)).to(dev)
    offsets = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int64, device=dev)
    total, B, V = int(pts.shape[0]), len(sizes), nx * ny * nz
    print(f"grid: {total} points in {B} tiles at {DIMS}", flush=True)
    desc, _ = _hip.voxel_prepare(pts, offsets, DIMS, regular=True)
    grid = torch.empty((B, 1, nz, nx, ny), dtype=torch.float64, device=dev)
    unb = torch.empty(B, dtype=torch.int64, device=dev)
    nans = torch.empty(B, dtype=torch.int64, device=dev)
    counts = torch.empty((B, nz, nx, ny), dtype=torch.int32, device=dev)
    towers = torch.empty((B, nz, nx, ny), dtype=torch.int32, device=dev)
    dropped = torch.empty(B, dtype=torch.int32, device=dev)

    def yard():
        _hip.voxel_scatter(pts, lab, offsets, desc, DIMS, [15.0], want_towers=True, counts=counts, towers=towers,
                           dropped=dropped)
        _hip.voxel_finalize(counts, towers, want_gt=True, want_occ=False)

    mine = lambda: _hip.voxel_classes(pts, lab, offsets, desc, DIMS, grid, unb, nans)               # noqa: E731
    noskip = lambda: _hip.voxel_classes(pts, lab, offsets, desc, DIMS, grid, unb, nans, skip=False)  # noqa: E731

    # what is timed is right: against scatter_reduce(amax) on the same flat indices, and both variants agree
    flat = flat_index_torch(pts, offsets, desc)
    want = torch.zeros(B * V, dtype=torch.float64, device=dev).scatter_reduce_(0, flat, lab, "amax", include_self=False)
    mine()
    assert torch.equal(grid.view(-1).view(torch.int64), want.view(torch.int64)) and int(unb.sum()) == 0
    occupied = int((want != 0).sum())
    noskip()
    assert torch.equal(grid.view(-1).view(torch.int64), want.view(torch.int64))

    def torch_grid():
        g = torch.zeros(B * V, dtype=torch.float64, device=dev)
        return g.scatter_reduce_(0, flat, lab, "amax", include_self=False)

    res = {"points": total, "tiles": B, "grid": list(DIMS), "occupied_voxels": occupied,
           "rows_per_occupied_voxel": round(total / occupied, 1),
           "yardstick_scatter_towers_finalize_gt": both_ways(yard, args.iters),
           "voxel_classes": both_ways(mine, args.iters), "voxel_classes_no_skip": both_ways(noskip, args.iters)}
    res["against_the_mark"] = verdict(res["voxel_classes"], res["yardstick_scatter_towers_finalize_gt"])
    res["skip_load_gain"] = round(res["voxel_classes_no_skip"]["graph_replay_us"] / res["voxel_classes"]["graph_replay_us"], 3)
    bytes_moved = total * 32 + B * V * 8 * 3
    res["bytes_moved"] = bytes_moved
    res["hbm_share_of_peak"] = round(bytes_moved / (res["voxel_classes"]["graph_replay_us"] * 1e-6) / HBM_PEAK, 3)
    t_torch = timed(torch_grid, max(2, args.iters // 2))
    t_index = timed(lambda: flat_index_torch(pts, offsets, desc), 2)
    m = min(args.host_points, sizes[0])
    loop = grid_host_loop(tiles[0][:m], labels[0][:m], desc[0].cpu().numpy())
    res["baselines"] = {"torch_scatter_reduce_amax_us": round(t_torch * 1e3, 1),
                        "torch_flat_index_us": round(t_index * 1e3, 1),
                        "torch_over_replay": round(t_torch * 1e3 / res["voxel_classes"]["graph_replay_us"], 2),
                        "torch_note": "scatter_reduce alone, the flat indices given; building them in torch is torch_flat_index_us",
                        "host_loop_points_timed": m, "host_loop_timed_ms": round(loop * 1e3, 1),
                        "host_loop_scaled_ms": round(loop * 1e3 * total / m, 1),
                        "host_loop_note": "timed on host_loop_points_timed points of one tile and scaled linearly to the batch",
                        "host_over_replay": round(loop * total / m * 1e6 / res["voxel_classes"]["graph_replay_us"], 1)}
    print(json.dumps(res, indent=1), flush=True)
    return res


# ---------------------------------------------------------------- class colours
def colour_host_loop(classes, class_color):
    """seconds of the reference's loop (pcd_processing.py:555-564)"""
    t0 = time.perf_counter()
    unique_classes = np.unique(classes)
    np_colors = np.empty((len(classes), 3))
    for i, c in enumerate(classes):
        np_colors[i, :] = class_color[np.where(unique_classes == c)[0][0]]
    return time.perf_counter() - t0


def colour_case(args):
    dev = torch.device("cuda:0")
    _, lab, _ = synthetic_scan(args.points)
    n = len(lab)
    print(f"colours: {n} classes, {len(np.unique(lab))} distinct", flush=True)
    cls = torch.from_numpy(lab).to(dev)
    offsets = torch.tensor([0, n], dtype=torch.int64, device=dev)
    table_np = np.random.default_rng(5).integers(0, 256, (22, 3)) / 255
    table = torch.from_numpy(table_np).to(dev)
    present = torch.empty((1, _hip.SN_CLASS_WORDS), dtype=torch.int32, device=dev)
    one = lambda: torch.empty(1, dtype=torch.int64, device=dev)   # noqa: E731
    bad, n_unique, short = one(), one(), one()
    unique = torch.empty((1, 22), dtype=torch.float64, device=dev)
    colors = torch.empty((n, 3), dtype=torch.float64, device=dev)
    rgb = torch.empty((n, 3), dtype=torch.int16, device=dev)
    census = lambda: _hip.class_census(cls, offsets, present, bad)                                                 # noqa: E731
    paint_c = lambda: _hip.class_paint(cls, offsets, present, table, colors, None, unique, n_unique, short)        # noqa: E731
    paint_r = lambda: _hip.class_paint(cls, offsets, present, table, None, rgb, unique, n_unique, short)           # noqa: E731

    def both_c():
        census()
        paint_c()

    def both_r():
        census()
        paint_r()

    def torch_colors():
        u = torch.unique(cls)
        return table.index_select(0, torch.searchsorted(u, cls))

    both_c()
    paint_r()
    want = torch_colors()
    assert torch.equal(colors.view(torch.int64), want.view(torch.int64)) and int(bad) == 0 and int(short) == 0
    q = torch.clamp(torch.round(255.0 * want), 0, 255).to(torch.int32) * 257
    assert torch.equal(rgb.to(torch.int32) & 0xffff, q)
    src = {k: torch.empty(n * k, dtype=torch.uint8, device=dev).random_(0, 256) for k in (20, 11)}
    dst = {k: torch.empty(n * k, dtype=torch.uint8, device=dev) for k in (20, 11)}
    res = {"classes": n, "distinct": int(n_unique), "table_rows": 22,
           "census": both_ways(census, args.iters), "paint_colors": both_ways(paint_c, args.iters),
           "paint_rgb": both_ways(paint_r, args.iters),
           "census_paint_colors": both_ways(both_c, args.iters), "census_paint_rgb": both_ways(both_r, args.iters),
           "yardstick_copy_20B_per_row": both_ways(lambda: dst[20].copy_(src[20]), args.iters),
           "yardstick_copy_11B_per_row": both_ways(lambda: dst[11].copy_(src[11]), args.iters)}
    res["against_the_mark_colors"] = verdict(res["census_paint_colors"], res["yardstick_copy_20B_per_row"])
    res["against_the_mark_rgb"] = verdict(res["census_paint_rgb"], res["yardstick_copy_11B_per_row"])
    for form, per_row in (("colors", 40), ("rgb", 22)):
        res[f"hbm_share_of_peak_{form}"] = round(n * per_row / (res[f"census_paint_{form}"]["graph_replay_us"] * 1e-6) / HBM_PEAK, 3)
    t_torch = timed(torch_colors, max(2, args.iters // 2))
    m = min(args.host_points, n)
    loop = colour_host_loop(lab[:: max(1, n // m)][:m], table_np)
    res["baselines"] = {"torch_unique_searchsorted_index_select_us": round(t_torch * 1e3, 1),
                        "torch_over_replay_colors": round(t_torch * 1e3 / res["census_paint_colors"]["graph_replay_us"], 2),
                        "host_loop_points_timed": m, "host_loop_timed_ms": round(loop * 1e3, 1),
                        "host_loop_scaled_ms": round(loop * 1e3 * n / m, 1),
                        "host_loop_note": "timed on host_loop_points_timed classes and scaled linearly to the scan",
                        "host_over_replay_colors": round(loop * n / m * 1e6 / res["census_paint_colors"]["graph_replay_us"], 1)}
    print(json.dumps(res, indent=1), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="voxel_classes_bench.json")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--tile-points", type=int, default=100_000)
    ap.add_argument("--host-points", type=int, default=100_000, help="points the host loops run (scaled to the input)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("voxel_classes_bench needs a HIP device (there is no CPU path)")
    res = {"device": torch.cuda.get_device_name(0), "grid_chunk_points": _hip.voxel_classes_chunk_points(),
           "class_chunk_points": _hip.class_chunk_points(), "hbm_peak_bytes_per_s": HBM_PEAK, "allowance": ALLOWANCE,
           "iters": args.iters}
    res["grid_c2"] = grid_case(args)
    res["colours"] = colour_case(args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
