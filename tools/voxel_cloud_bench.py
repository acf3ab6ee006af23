#!/usr/bin/env python3
"""K16 voxel clouds on 32 grids of 64^3 (f32) at the live fractions 1 %, 10 % and 50 %, in both colour modes.  Timed between
HIP events after a warm-up: sn_voxel_cloud_count, sn_voxel_cloud_scatter (rows, exact capacity), and the two captured into a
hipGraph and replayed.  Baselines that need none of this library's kernels: the torch-on-device formulation (nonzero, index,
the colour rule / table lookup) and the reference-shaped numpy loop on the host (a Python loop over the voxels and an np.where
per voxel, timed on the first voxels of one tile and scaled), including the copy of the grids down.
Yardstick: sn_grid_to_points on the same grids in the same run -- the one kernel of the library that turns cells into rows; it
writes every cell.  Its achieved bytes per second, applied to the bytes count + scatter move, plus 25 % for the prefix pass
the compaction adds, is the mark; the JSON says on which side of it each case lands.
Bytes are the algorithm's: 4 B per cell and pass, 48 B written per live cell, the workspace once each way.
The bench checks what it times: offsets and rows against the torch formulation.  Writes one JSON file.
    python tools/voxel_cloud_bench.py --out profiles/voxel_cloud_bench.json [--iters 50]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/voxel_cloud_bench.py --trace ranges 0.01    # time per kernel"""
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
from scene_net_amd.voxel_cloud import jet_ranges  # noqa: E402

B, N = 32, 64
HBM_PEAK = 8.0e12      # bytes / s, the part's specification
ALLOWANCE = 1.25
R = 10


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


def make_grids(fraction, mode, seed):
    """[B, N, N, N] f32: `fraction` of the cells live under `mode`, the rest zero"""
    rng = np.random.default_rng(seed)
    v = rng.uniform(0.12, 1.0, (B, N, N, N)) if mode == "ranges" else rng.uniform(-1.0, 1.0, (B, N, N, N))
    v[rng.random((B, N, N, N)) >= fraction] = 0.0
    return v.astype(np.float32)


def torch_formulation(grids, mode, table255, lin, step):
    """what a user writes without the library: nonzero, index, the colour rule -> rows [total, 6] f64 and offsets"""
    v = grids.to(torch.float64)
    live = v > lin[1] if mode == "ranges" else v != 0
    idx = torch.nonzero(live)                       # (b, z, x, y) in C order
    c = v[idx[:, 0], idx[:, 1], idx[:, 2], idx[:, 3]]
    xyz = torch.stack([idx[:, 2], idx[:, 3], idx[:, 1]], dim=1).to(torch.float64)
    if mode == "ranges":
        rgb = table255[torch.argmin(torch.abs(c[:, None] - lin - step), dim=-1)]
    else:
        neg = c < 0
        ch = torch.where(neg, 1.0 + c, 1.0 - c) * 255.0
        full = torch.full_like(ch, 255.0)
        rgb = torch.stack([torch.where(neg, ch, full), ch, torch.where(neg, full, ch)], dim=1)
    counts = torch.bincount(idx[:, 0], minlength=grids.shape[0])
    offsets = torch.cat([counts.new_zeros(1), torch.cumsum(counts, 0)])
    return torch.cat([xyz, rgb], dim=1), offsets


def numpy_loop(grids_dev, mode, table, voxels):
    """seconds: the copy down, and the reference-shaped loop over the first `voxels` live voxels of tile 0, scaled to the
    live voxels of all tiles"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    host = grids_dev.cpu().numpy()
    d2h = time.perf_counter() - t0
    grid = host[0]
    t0 = time.perf_counter()
    z, x, y = grid.nonzero()
    xyz = np.empty((len(z), 4))
    for n, (i, j, k) in enumerate(zip(x, y, z)):
        xyz[n] = [int(i), int(j), int(k), grid[k, i, j]]
    head = time.perf_counter() - t0
    t0 = time.perf_counter()
    if mode == "ranges":
        lin, step = np.linspace(0, 1, R), (1 / R) / 2
        xyz = xyz[xyz[:, -1] > lin[1]]
        uq = np.unique(xyz[:, -1])
        colours = table[np.argmin(np.abs(np.expand_dims(uq, -1) - lin - step), axis=-1)]
    else:
        uq = np.unique(xyz[:, -1])
        colours = np.array([[1 + c, 1 + c, 1] if c < 0 else [1, 1 - c, 1 - c] for c in uq])
    rule = time.perf_counter() - t0
    m = min(voxels, len(xyz))
    out = np.empty((m, 3))
    t0 = time.perf_counter()
    for n, c in enumerate(xyz[:m, -1]):
        out[n, :] = colours[np.where(uq == c)[0][0]]
    lookup = (time.perf_counter() - t0) * len(xyz) / max(m, 1)
    return d2h, (head + rule + lookup) * grids_dev.shape[0], m


def case(name, fraction, mode, iters, host_voxels, g2p_rate):
    dev = torch.device("cuda:0")
    grids = torch.from_numpy(make_grids(fraction, mode, seed=int(fraction * 1000))).to(dev)
    cells = grids.numel()
    V = N * N * N
    m = _hip.SN_CLOUD_RANGES if mode == "ranges" else _hip.SN_CLOUD_DENSITY
    table = jet_ranges(R) if mode == "ranges" else None
    ws = torch.empty(_hip.voxel_cloud_ws_bytes(B, V) // 8, dtype=torch.int64, device=dev)
    offsets = torch.empty(B + 1, dtype=torch.int64, device=dev)
    bad = torch.empty((B, 2), dtype=torch.int64, device=dev)
    _hip.voxel_cloud_count(grids, m, R, None, ws, offsets, bad)
    total = int(offsets[-1])
    rows = torch.empty((total, 6), dtype=torch.float64, device=dev)

    def count():
        _hip.voxel_cloud_count(grids, m, R, None, ws, offsets, bad)

    def scatter():
        _hip.voxel_cloud_scatter(grids, m, R, table, None, ws, offsets, rows)

    def both():
        count()
        scatter()
    both()
    lin = torch.from_numpy(np.linspace(0, 1, R)).to(dev)
    table255 = torch.from_numpy(jet_ranges(R) * 255.0).to(dev)
    step = (1 / R) / 2
    want, want_off = torch_formulation(grids, mode, table255, lin, step)
    assert offsets.tolist() == want_off.tolist()
    assert torch.equal(rows.view(torch.int64), want.contiguous().view(torch.int64)), "rows differ from the torch formulation"
    del want, want_off
    t_count, t_scatter, t_both = timed(count, iters), timed(scatter, iters), timed(both, iters)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        both()
    t_replay = timed(graph.replay, iters)
    del graph
    t_torch = timed(lambda: torch_formulation(grids, mode, table255, lin, step), max(2, iters // 5))
    d2h, loop, timed_voxels = numpy_loop(grids, mode, jet_ranges(R), host_voxels)
    ws_bytes = ws.numel() * 8
    count_bytes = cells * 4 + ws_bytes
    scatter_bytes = cells * 4 + total * 48 + ws_bytes
    mark_us = (count_bytes + scatter_bytes) / g2p_rate * ALLOWANCE * 1e6
    res = {"case": name, "mode": mode, "live_fraction": fraction, "rows_out": total,
           "count_us": round(t_count * 1e3, 1), "scatter_us": round(t_scatter * 1e3, 1),
           "count_then_scatter_us": round(t_both * 1e3, 1), "graph_replay_us": round(t_replay * 1e3, 1),
           "count_bytes": count_bytes, "scatter_bytes": scatter_bytes,
           "count_hbm_share": round(count_bytes / (t_count * 1e-3) / HBM_PEAK, 3),
           "scatter_hbm_share": round(scatter_bytes / (t_scatter * 1e-3) / HBM_PEAK, 3),
           "yardstick_mark_us": round(mark_us, 1), "replay_over_mark": round(t_replay * 1e3 / mark_us, 2),
           "within_mark": bool(t_replay * 1e3 <= mark_us),
           "torch_formulation_us": round(t_torch * 1e3, 1), "torch_over_replay": round(t_torch / t_replay, 2),
           "host_copy_down_ms": round(d2h * 1e3, 1), "host_numpy_loop_ms": round(loop * 1e3, 1),
           "host_voxels_timed": timed_voxels, "host_over_replay": round((d2h + loop) * 1e3 / t_replay, 1)}
    print(f"{name:22s} rows {total:8d}  count {res['count_us']:7.1f} us ({res['count_hbm_share']:.2f} of HBM peak)  "
          f"scatter {res['scatter_us']:7.1f} us ({res['scatter_hbm_share']:.2f})  replay {res['graph_replay_us']:7.1f} us  "
          f"mark {res['yardstick_mark_us']:7.1f} us ({res['replay_over_mark']:.2f})  torch {res['torch_formulation_us']:9.1f} us  "
          f"host {res['host_copy_down_ms'] + res['host_numpy_loop_ms']:9.1f} ms", flush=True)
    return res


def trace(mode, fraction, calls=200):
    dev = torch.device("cuda:0")
    grids = torch.from_numpy(make_grids(fraction, mode, seed=int(fraction * 1000))).to(dev)
    m = _hip.SN_CLOUD_RANGES if mode == "ranges" else _hip.SN_CLOUD_DENSITY
    table = jet_ranges(R) if mode == "ranges" else None
    ws = torch.empty(_hip.voxel_cloud_ws_bytes(B, N * N * N) // 8, dtype=torch.int64, device=dev)
    offsets = torch.empty(B + 1, dtype=torch.int64, device=dev)
    bad = torch.empty((B, 2), dtype=torch.int64, device=dev)
    _hip.voxel_cloud_count(grids, m, R, None, ws, offsets, bad)
    rows = torch.empty((int(offsets[-1]), 6), dtype=torch.float64, device=dev)
    flat = grids.reshape(B * N, N, N)
    out = torch.empty((flat.numel(), 4), dtype=torch.float64, device=dev)
    for _ in range(calls):
        _hip.voxel_cloud_count(grids, m, R, None, ws, offsets, bad)
        _hip.voxel_cloud_scatter(grids, m, R, table, None, ws, offsets, rows)
        assert _hip.load().sn_grid_to_points(flat.data_ptr(), _hip.SN_F32, B * N, N, N, None, None, out.data_ptr(),
                                             _hip._stream()) == 0
    torch.cuda.synchronize()


def yardstick(iters):
    """sn_grid_to_points over the same 32 x 64^3 cells (one [B * N, N, N] grid): bytes per second it achieves"""
    dev = torch.device("cuda:0")
    grid = torch.from_numpy(make_grids(0.1, "density", seed=1)).to(dev).reshape(B * N, N, N)
    _hip.grid_to_points(grid)
    t = timed(lambda: _hip.grid_to_points(grid), iters)       # (allocates its output like every call of it does)
    out = torch.empty((grid.numel(), 4), dtype=torch.float64, device=dev)

    def raw():
        rc = _hip.load().sn_grid_to_points(grid.data_ptr(), _hip.SN_F32, B * N, N, N, None, None, out.data_ptr(), _hip._stream())
        assert rc == 0
    t_raw = timed(raw, iters)
    nbytes = grid.numel() * (4 + 32)
    return {"grid_to_points_us": round(t_raw * 1e3, 1), "grid_to_points_with_allocation_us": round(t * 1e3, 1),
            "bytes": nbytes, "bytes_per_s": nbytes / (t_raw * 1e-3), "hbm_share": round(nbytes / (t_raw * 1e-3) / HBM_PEAK, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="voxel_cloud_bench.json")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--host-voxels", type=int, default=20000, help="voxels the numpy lookup loop runs (scaled to all)")
    ap.add_argument("--trace", nargs=2, metavar=("MODE", "FRACTION"),
                    help="the program for rocprofv3 --kernel-trace --stats: count + scatter of one case, 200 times, nothing timed")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("voxel_cloud_bench needs a HIP device (there is no CPU path)")
    dev = torch.device("cuda:0")
    if args.trace:
        trace(args.trace[0], float(args.trace[1]))
        return
    y = yardstick(args.iters)
    print(f"yardstick sn_grid_to_points: {y['grid_to_points_us']} us for {y['bytes']} bytes ({y['hbm_share']} of HBM peak)", flush=True)
    res = {"device": torch.cuda.get_device_name(dev), "grids": [B, N, N, N], "dtype": "float32", "r": R,
           "chunk_cells": _hip.voxel_cloud_chunk_cells(), "hbm_peak_bytes_per_s": HBM_PEAK, "allowance": ALLOWANCE,
           "yardstick": y, "cases": []}
    for mode in ("density", "ranges"):
        for fraction in (0.01, 0.10, 0.50):
            res["cases"].append(case(f"{mode} {int(fraction * 100)} % live", fraction, mode, args.iters, args.host_voxels,
                                     y["bytes_per_s"]))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
