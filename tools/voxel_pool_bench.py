#!/usr/bin/env python3
"""K24 on the C2 batch (32 tiles of 10^5 points, 64^3).  Timed between HIP events after a warm-up, eager and captured into a
hipGraph and replayed.
sn_voxel_pool at P = 1 (z.mean), P = 3 (the centroids) and P = 8 (mean, min and max of z and of a value column, min of x, max
of y), and -- where a plane is a minimum or a maximum -- with and without the look before the atomic.  (The accumulators
live in the outputs; the other layout that was built, a workspace interleaved per voxel, is on record in
profiles/voxel_pool_layouts_bench.json, measured by this tool before that layout was taken out.)
Yardstick, measured in the same run: sn_voxel_classes with SN_VOXEL_CLASSES_NO_SKIP on the same batch -- it clears, sends one
64-bit atomic per row for, and decodes ONE f64 plane; a pooling call does that for P planes and the counts, so the yardstick
is that time times P + 1 and the mark that product plus 25 %.
Baselines that need none of this library's kernels: the torch formulation on the device (index_add_ for the sums and the
counts, scatter_reduce amin / amax for the extrema, the flat indices GIVEN) and np.add.at on the host, timed on 10^5 points
of one tile and SCALED linearly to the batch.
The bench checks what it times: the counts against index_add_ exactly, the centroids against the torch fp64 mean within the
documented span * 2^-32, the extrema bit for bit, and the call without the look against the one with it bit for bit.  Writes
one JSON file.
    python tools/voxel_pool_bench.py --out profiles/voxel_pool_bench.json [--iters 20] [--cases P3_centroids]"""
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
from crops_bench import HBM_PEAK, timed  # noqa: E402
from voxel_classes_bench import ALLOWANCE, both_ways, flat_index_torch  # noqa: E402
from scene_net_amd import _hip  # noqa: E402
from scene_net_amd.synthetic import synthetic_tile  # noqa: E402

DIMS = (64, 64, 64)
MEAN, MIN, MAX = _hip.SN_POOL_MEAN, _hip.SN_POOL_MIN, _hip.SN_POOL_MAX
CASES = {"P1_z_mean": ([2], [MEAN]),
         "P3_centroids": ([0, 1, 2], [MEAN, MEAN, MEAN]),
         "P8_mixed": ([2, 2, 2, 3, 3, 3, 0, 1], [MEAN, MIN, MAX, MEAN, MIN, MAX, MIN, MAX])}
RANGE = [(0.0, 1.0)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/voxel_pool_bench.json")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--tile-points", type=int, default=100_000)
    ap.add_argument("--host-points", type=int, default=100_000)
    ap.add_argument("--cases", default=",".join(CASES), help="comma-separated subset of " + ", ".join(CASES))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    nx, ny, nz = DIMS
    tiles, labels = zip(*[synthetic_tile(t, args.tile_points) for t in range(args.batch)])
    sizes = [len(t) for t in tiles]
    pts = torch.from_numpy(np.concatenate(tiles)).to(dev)
    lab = torch.from_numpy(np.concatenate(labels)).to(dev)
    rng = np.random.default_rng(24)
    val = torch.from_numpy(rng.random((int(pts.shape[0]), 1))).to(dev)             # a feature in [0, 1): K22's kind
    offsets = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int64, device=dev)
    total, B, V = int(pts.shape[0]), len(sizes), nx * ny * nz
    print(f"{total} points in {B} tiles at {DIMS}", flush=True)
    desc, _ = _hip.voxel_prepare(pts, offsets, DIMS, regular=True)
    flat = flat_index_torch(pts, offsets, desc)
    unb = torch.empty(B, dtype=torch.int64, device=dev)
    nans = torch.empty(B, dtype=torch.int64, device=dev)
    counts = torch.empty((B, nz, nx, ny), dtype=torch.int32, device=dev)
    grid = torch.empty((B, 1, nz, nx, ny), dtype=torch.float64, device=dev)

    yard = lambda: _hip.voxel_classes(pts, lab, offsets, desc, DIMS, grid, unb, nans, skip=False)   # noqa: E731
    res = {"device": torch.cuda.get_device_name(0), "chunk_points": _hip.voxel_pool_chunk_points(), "allowance": ALLOWANCE,
           "iters": args.iters, "points": total, "tiles": B, "grid": list(DIMS),
           "yardstick_voxel_classes_no_skip": both_ways(yard, args.iters), "cases": {}}
    y_us = res["yardstick_voxel_classes_no_skip"]["graph_replay_us"]
    want_counts = torch.zeros(B * V, dtype=torch.int32, device=dev).index_add_(
        0, flat, torch.ones(total, dtype=torch.int32, device=dev))
    res["occupied_voxels"] = int((want_counts > 0).sum())
    res["rows_per_occupied_voxel"] = round(total / res["occupied_voxels"], 1)
    columns = [pts[:, 0].contiguous(), pts[:, 1].contiguous(), pts[:, 2].contiguous(), val[:, 0].contiguous()]
    span = (desc[:, 3:6] - desc[:, 0:3]).max().item()

    for name in args.cases.split(","):
        src, ops = CASES[name]
        P = len(src)
        out = torch.empty((B, P, nz, nx, ny), dtype=torch.float64, device=dev)
        out2 = torch.empty_like(out)
        values = val if any(s >= 3 for s in src) else None
        ranges = RANGE if values is not None else None

        def call(o, look=True):
            _hip.voxel_pool(pts, values, offsets, desc, DIMS, src, ops, ranges, 0.0, o, counts, unb, nans, look=look)

        # what is timed is right
        call(out)
        assert torch.equal(counts.view(-1), want_counts) and int(unb.sum()) == 0 and int(nans.sum()) == 0
        call(out2, look=False)
        assert torch.equal(out.view(torch.int64), out2.view(torch.int64)) and torch.equal(counts.view(-1), want_counts)
        hit = want_counts > 0
        for p, (s, op) in enumerate(zip(src, ops)):
            got = out[:, p].reshape(-1)
            if op == MEAN:
                mean = torch.zeros(B * V, dtype=torch.float64, device=dev).index_add_(0, flat, columns[s]) / want_counts
                tol = (span if s < 3 else 1.0) * 2.0 ** -32 + 1e-6
                assert float((got[hit] - mean[hit]).abs().max()) <= tol, (name, p)
            else:
                ext = torch.zeros(B * V, dtype=torch.float64, device=dev).scatter_reduce_(
                    0, flat, columns[s], "amin" if op == MIN else "amax", include_self=False)
                assert torch.equal(got[hit].view(torch.int64), ext[hit].view(torch.int64)), (name, p)

        def torch_pool():
            n = torch.zeros(B * V, dtype=torch.int32, device=dev).index_add_(0, flat, torch.ones(total, dtype=torch.int32,
                                                                                               device=dev))
            planes = []
            for s, op in zip(src, ops):
                if op == MEAN:
                    planes.append(torch.zeros(B * V, dtype=torch.float64, device=dev).index_add_(0, flat, columns[s]) / n)
                else:
                    planes.append(torch.zeros(B * V, dtype=torch.float64, device=dev).scatter_reduce_(
                        0, flat, columns[s], "amin" if op == MIN else "amax", include_self=False))
            return planes

        case = {"planes": P, "voxel_pool": both_ways(lambda: call(out), args.iters)}
        if any(op != MEAN for op in ops):
            case["voxel_pool_no_look"] = both_ways(lambda: call(out, look=False), args.iters)
            case["look_gain"] = round(case["voxel_pool_no_look"]["graph_replay_us"] / case["voxel_pool"]["graph_replay_us"], 3)
        t = case["voxel_pool"]["graph_replay_us"]
        mark = round(y_us * (P + 1) * ALLOWANCE, 1)
        case["against_the_mark"] = {"graph_replay_us": t, "yardstick_times_planes_plus_one_us": round(y_us * (P + 1), 1),
                                    "mark_us": mark, "over_yardstick": round(t / (y_us * (P + 1)), 3),
                                    "position": "INSIDE" if t <= mark else "OUTSIDE"}
        case["bytes_moved"] = total * (24 + (8 if values is not None else 0)) + B * V * (P * 8 + 4) * 3
        case["hbm_share_of_peak"] = round(case["bytes_moved"] / (t * 1e-6) / HBM_PEAK, 3)
        t_torch = timed(torch_pool, max(2, args.iters // 2))
        case["torch_index_add_scatter_reduce_us"] = round(t_torch * 1e3, 1)
        case["torch_over_replay"] = round(t_torch * 1e3 / t, 2)
        res["cases"][name] = case
        print(name, json.dumps(case), flush=True)
        del out, out2

    # the host: np.add.at of one column and the counts on one tile's points, the flat indices given
    m = min(args.host_points, sizes[0])
    f_host = flat[:m].cpu().numpy()
    z_host = tiles[0][:m, 2].copy()
    t0 = time.perf_counter()
    s_host, n_host = np.zeros(V), np.zeros(V, dtype=np.int64)
    np.add.at(s_host, f_host, z_host)
    np.add.at(n_host, f_host, 1)
    host = time.perf_counter() - t0
    res["baselines"] = {"torch_flat_index_us": round(timed(lambda: flat_index_torch(pts, offsets, desc), 2) * 1e3, 1),
                        "torch_note": "index_add_ / scatter_reduce alone, the flat indices given; building them in torch is "
                                      "torch_flat_index_us",
                        "host_add_at_points_timed": m, "host_add_at_one_plane_ms": round(host * 1e3, 1),
                        "host_add_at_one_plane_scaled_ms": round(host * 1e3 * total / m, 1),
                        "host_note": "np.add.at of one column and the counts on host_add_at_points_timed points of one tile, "
                                     "scaled linearly to the batch; a call of P planes makes P + 1 such passes"}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res["yardstick_voxel_classes_no_skip"]), "->", args.out, flush=True)


if __name__ == "__main__":
    main()
