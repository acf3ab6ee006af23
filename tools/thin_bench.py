#!/usr/bin/env python3
"""K17 thinning on one synthetic scan of 10^7 points (crops_bench's scan) and on a batch of 32 tiles of 10^5 points.  Timed
between HIP events after a warm-up: sn_thin_count, sn_thin_scatter (labels and src, exact capacity) and the two captured
into a hipGraph and replayed -- keep 1.0 / 0.8 / 0.5, group none / z / voxel at 64^3, explicit uniforms against the
built-in generator; for the grouped rules also the count with `first` (the atomics) and the scatter that decides again
(out_key).
Yardstick, measured in the same run: sn_crop_count + sn_crop_scatter with ONE box that admits every point, labels and src
-- the same 32 B read and 40 B written per row as thinning at keep 1.0 without groups.  The mark is that time plus 25 %.
Baselines that need none of this library's kernels: the same rule through torch on the device (rand, compare, nonzero,
index_select) and the reference-shaped Python loop on the host (dict of lists by voxel, np.random.rand per group), timed
on 10^5 points and SCALED linearly to the input's size, plus the copy of the input down.
The bench checks what it times: the kept count against torch's on the same uniforms.  Writes one JSON file.
    python tools/thin_bench.py --out profiles/thin_bench.json [--iters 20]"""
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
GROUPS = (("none", _hip.SN_THIN_GROUP_NONE), ("z", _hip.SN_THIN_GROUP_Z), ("voxel", _hip.SN_THIN_GROUP_VOXEL))
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


def yardstick(pts, labels, iters):
    """us: count, scatter and the replayed pair of K9 with one box that admits every point (labels and src)"""
    dev, n = pts.device, pts.shape[0]
    inf = float("inf")
    regions = torch.tensor([[-inf, -inf, inf, inf]], dtype=torch.float64, device=dev)
    kinds = torch.full((1,), _hip.SN_CROP_BOX, dtype=torch.int32, device=dev)
    ws = torch.empty(_hip.crops_ws_bytes(n, 1) // 8, dtype=torch.int64, device=dev)
    offsets = torch.empty(2, dtype=torch.int64, device=dev)
    out_pts = torch.empty((n, 3), dtype=torch.float64, device=dev)
    out_lab = torch.empty((n,), dtype=torch.float64, device=dev)
    out_src = torch.empty((n,), dtype=torch.int64, device=dev)
    count = lambda: _hip.crop_count(pts, regions, kinds, ws, offsets)   # noqa: E731
    scatter = lambda: _hip.crop_scatter(pts, labels, regions, kinds, ws, offsets, out_pts, out_lab, out_src)   # noqa: E731

    def both():
        count()
        scatter()
    both()
    assert int(offsets[-1]) == n and torch.equal(out_pts.view(torch.int64), pts.view(torch.int64))
    return {"count_us": round(timed(count, iters) * 1e3, 1), "scatter_us": round(timed(scatter, iters) * 1e3, 1),
            "graph_replay_us": round(replayed(both, iters) * 1e3, 1)}


def thin_case(pts, labels, offsets, desc, u_all, group, kind, keep, source, iters):
    dev, n, B = pts.device, pts.shape[0], offsets.numel() - 1
    G = _hip.thin_groups(kind, DIMS)
    thr = torch.full((B, G), keep, dtype=torch.float64, device=dev)
    seed = torch.tensor([0x1234567 + 1], dtype=torch.int64, device=dev) if source == "seed" else None
    u = u_all if source == "u" else None
    d = desc if kind != _hip.SN_THIN_GROUP_NONE else None
    ws = torch.empty(_hip.thin_ws_bytes(n, B) // 8, dtype=torch.int64, device=dev)
    offsets_out = torch.empty(B + 1, dtype=torch.int64, device=dev)
    unbinned = torch.empty(B, dtype=torch.int64, device=dev)
    rule = (offsets, kind, d, DIMS, thr, u, seed, None, ws)
    _hip.thin_count(pts, *rule, offsets_out, unbinned, None)
    rows = int(offsets_out[-1])
    if source == "u":
        assert rows == int((u_all <= keep).sum()) and int(unbinned.sum()) == 0
    out_pts = torch.empty((rows, 3), dtype=torch.float64, device=dev)
    out_lab = torch.empty((rows,), dtype=torch.float64, device=dev)
    out_src = torch.empty((rows,), dtype=torch.int64, device=dev)
    count = lambda: _hip.thin_count(pts, *rule, offsets_out, unbinned, None)   # noqa: E731
    scatter = lambda: _hip.thin_scatter(pts, labels, *rule, out_pts, out_lab, out_src, None)   # noqa: E731

    def both():
        count()
        scatter()
    both()
    if keep == 1.0:
        assert rows == n and torch.equal(out_pts.view(torch.int64), pts.view(torch.int64))
    t_count, t_scatter, t_replay = timed(count, iters), timed(scatter, iters), replayed(both, iters)
    grouped = kind != _hip.SN_THIN_GROUP_NONE
    count_bytes = n * ((8 if source == "u" else 0) + (24 + 8 if grouped else 0)) + n // 4
    scatter_bytes = rows * (32 + 40) + n // 8
    res = {"group": group, "keep": keep, "uniform": source, "rows_out": rows,
           "count_us": round(t_count * 1e3, 1), "scatter_us": round(t_scatter * 1e3, 1),
           "graph_replay_us": round(t_replay * 1e3, 1), "count_bytes": count_bytes, "scatter_bytes": scatter_bytes,
           "scatter_hbm_share": round(scatter_bytes / (t_scatter * 1e-3) / HBM_PEAK, 3)}
    if grouped:
        first = torch.empty((B, G), dtype=torch.int64, device=dev)
        out_key = torch.empty((rows,), dtype=torch.int32, device=dev)
        res["count_with_first_us"] = round(timed(lambda: _hip.thin_count(pts, *rule, offsets_out, unbinned, first), iters) * 1e3, 1)
        res["scatter_with_key_us"] = round(
            timed(lambda: _hip.thin_scatter(pts, labels, *rule, out_pts, out_lab, out_src, out_key), iters) * 1e3, 1)
    print(f"  {group:5s} keep {keep:.1f} {source:4s} rows {rows:9d}  count {res['count_us']:8.1f} us  scatter "
          f"{res['scatter_us']:8.1f} us ({res['scatter_hbm_share']:.2f} of HBM peak)  replay {res['graph_replay_us']:8.1f} us",
          flush=True)
    return res


def torch_formulation(pts, labels, keep):
    idx = torch.nonzero(torch.rand(pts.shape[0], dtype=torch.float64, device=pts.device) <= keep).reshape(-1)
    return pts.index_select(0, idx), labels.index_select(0, idx), idx


def host_loop(xyz, classes, desc_row, samp_per):
    """seconds of the reference-shaped downsampling loop (pcd_processing.py:399-420) on the host, voxel indices given"""
    nx, ny, nz = DIMS
    e = [desc_row[6:6 + nx + 1], desc_row[6 + nx + 1:6 + nx + ny + 2], desc_row[6 + nx + ny + 2:]]
    ix, iy, iz = (np.clip(np.searchsorted(e[a], xyz[:, a], side="left") - 1, 0, DIMS[a] - 1) for a in range(3))
    voxel_n = (iz * nx + ix) * ny + iy
    t0 = time.perf_counter()
    voxels = dict()
    for i, point in enumerate(xyz):
        idx = voxel_n[i]
        vox = voxels.get(idx, list())
        vox.append(int(i))
        voxels[idx] = vox
    used_voxels = np.fromiter(voxels.keys(), dtype=int)
    sampling = np.zeros(len(xyz))
    counter = 0
    for vox in used_voxels:
        npvox = np.array(voxels[vox])
        selected = np.random.rand(len(npvox))
        sample = npvox[selected <= samp_per]
        end = counter + len(sample)
        sampling[counter:end] = sample
        counter = end
    sampling = sampling[:counter].astype(int)
    xyz[sampling], classes[sampling]
    return time.perf_counter() - t0


def input_case(name, xyz_tiles, lab_tiles, iters, host_points):
    dev = torch.device("cuda:0")
    sizes = [len(t) for t in xyz_tiles]
    pts = torch.from_numpy(np.concatenate(xyz_tiles)).to(dev)
    labels = torch.from_numpy(np.concatenate(lab_tiles)).to(dev)
    offsets = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int64, device=dev)
    n, B = int(pts.shape[0]), len(sizes)
    print(f"{name}: {n} points in {B} tile(s)", flush=True)
    desc, _ = _hip.voxel_prepare(pts, offsets, DIMS, regular=True)
    u_all = torch.rand(n, dtype=torch.float64, device=dev)
    res = {"input": name, "points": n, "tiles": B, "yardstick_crop_all": yardstick(pts, labels, iters), "cases": []}
    y = res["yardstick_crop_all"]
    y["mark_us"] = round(y["graph_replay_us"] * ALLOWANCE, 1)
    print(f"  yardstick (crop, one box, all rows): count {y['count_us']} us  scatter {y['scatter_us']} us  replay "
          f"{y['graph_replay_us']} us  -> mark {y['mark_us']} us", flush=True)
    for group, kind in GROUPS:
        for keep in (1.0, 0.8, 0.5):
            for source in ("u", "seed"):
                res["cases"].append(thin_case(pts, labels, offsets, desc, u_all, group, kind, keep, source, iters))
    verdicts = {}
    for c in res["cases"]:
        if c["group"] == "none" and c["keep"] == 1.0:
            verdicts[c["uniform"]] = {"graph_replay_us": c["graph_replay_us"],
                                      "over_yardstick": round(c["graph_replay_us"] / y["graph_replay_us"], 3),
                                      "position": "INSIDE" if c["graph_replay_us"] <= y["mark_us"] else "OUTSIDE"}
    res["against_the_mark_keep_1_group_none"] = verdicts
    print(f"  against the mark: {verdicts}", flush=True)
    base = {c["uniform"]: c["graph_replay_us"] for c in res["cases"] if c["group"] == "none" and c["keep"] == 0.5}
    t_torch = timed(lambda: torch_formulation(pts, labels, 0.5), max(2, iters // 2))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    xyz_h, cls_h = pts.cpu().numpy(), labels.cpu().numpy()
    d2h = time.perf_counter() - t0
    m = min(host_points, sizes[0])
    pick = slice(None, m) if B > 1 else slice(None, None, max(1, n // m))      # a tile, or the scan thinned to its size
    m = len(xyz_h[pick])
    loop = host_loop(xyz_h[pick], cls_h[pick], desc[0].cpu().numpy(), 0.5)
    res["baselines_keep_0.5"] = {"torch_formulation_us": round(t_torch * 1e3, 1),
                                 "torch_over_replay_seed": round(t_torch * 1e3 / base["seed"], 2),
                                 "host_copy_down_ms": round(d2h * 1e3, 1), "host_loop_points_timed": m,
                                 "host_loop_timed_ms": round(loop * 1e3, 1),
                                 "host_loop_scaled_ms": round(loop * 1e3 * n / m, 1),
                                 "host_loop_note": "timed on host_loop_points_timed points and scaled linearly to the input",
                                 "host_over_replay_seed": round((d2h + loop * n / m) * 1e6 / base["seed"], 1)}
    print(f"  baselines at keep 0.5: {res['baselines_keep_0.5']}", flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="thin_bench.json")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--tile-points", type=int, default=100_000)
    ap.add_argument("--host-points", type=int, default=100_000, help="points the host loop runs (scaled to the input)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("thin_bench needs a HIP device (there is no CPU path)")
    res = {"device": torch.cuda.get_device_name(0), "grid": list(DIMS), "chunk_points": _hip.thin_chunk_points(),
           "hbm_peak_bytes_per_s": HBM_PEAK, "allowance": ALLOWANCE, "inputs": []}
    xyz, lab, _ = synthetic_scan(args.points)
    res["inputs"].append(input_case("one scan", [xyz], [lab], args.iters, args.host_points))
    del xyz, lab
    tiles, labels = zip(*[synthetic_tile(t, args.tile_points) for t in range(args.batch)])
    res["inputs"].append(input_case("batch of tiles", list(tiles), list(labels), args.iters, args.host_points))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
