#!/usr/bin/env python3
"""K19 scan merge on tools/crops_bench.py's scan: 10^7 points, a 16 x 8 lattice of synthetic tiles, random f32 predictions at
64^3 for every region's tile.  Region sets: the 32-box lattice without overlap, 128 boxes with 5 m overlap, 128 discs of
15 m at the towers.  Timed between HIP events, every variant in turn within a round, the rounds repeated in the same
process after a warm-up; median and range over the rounds:
  * sn_scan_merge per rule, with and without cover, and (interior, cover) captured into a hipGraph and replayed;
  * the parent formulation on the same crops: sn_gather_points over the cropped rows + crops.merge_to_scan;
  * the yardstick: sn_crop_count on the same regions + sn_gather_points on the cropped rows -- the two reads the kernel
    fuses.  Their sum plus 25 % is the mark; a row says INSIDE or OUTSIDE.
The bench checks what it times: rule "max" against the parent formulation, bit for bit.
Kernel times are a run of their own: `rocprofv3 --kernel-trace --stats -d DIR -- python tools/scan_merge_bench.py --trace`
runs every kernel a few times on the 128-box set and nothing else; `--kernel-stats FILE` (the kernel_stats csv of that run)
puts its rows into the JSON.  Without it the JSON says the kernel times were not measured.
    python tools/scan_merge_bench.py --out profiles/scan_merge_bench.json [--rounds 7] [--iters 5]"""
import argparse
import csv
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import scene_net_amd as sna  # noqa: E402
from scene_net_amd import _hip  # noqa: E402
from scene_net_amd.crops import lattice_boxes  # noqa: E402
from crops_bench import synthetic_scan  # noqa: E402

GRID = (64, 64, 64)
RULES = (("max", _hip.SN_MERGE_MAX), ("mean", _hip.SN_MERGE_MEAN), ("interior", _hip.SN_MERGE_INTERIOR))
ALLOWANCE = 1.25


def once(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters       # us


def region_sets(xyz, towers):
    lo, hi = xyz[:, :2].min(axis=0), xyz[:, :2].max(axis=0)
    lattice = lattice_boxes(lo, hi, 60.0, overlap=0.0)
    overlap = lattice_boxes(lo, hi, 30.0, overlap=5.0)
    assert lattice.shape[0] == 32 and overlap.shape[0] == 128
    discs = np.column_stack([towers[:, :2], np.full(len(towers), 15.0), np.zeros(len(towers))])
    return [("32 boxes, no overlap", lattice, np.ones(32, dtype=np.int32)),
            ("128 boxes, 5 m overlap", overlap, np.ones(128, dtype=np.int32)),
            ("128 discs r=15", discs, np.zeros(len(discs), dtype=np.int32))]


class Case:
    def __init__(self, name, pts, regions_np, kinds_np):
        dev = pts.device
        self.name, self.pts, self.n, self.K = name, pts, int(pts.shape[0]), int(regions_np.shape[0])
        self.regions, self.kinds = torch.from_numpy(regions_np).to(dev), torch.from_numpy(kinds_np).to(dev)
        self.crops = sna.crop_regions(pts, self.regions, self.kinds)
        self.batch, self.kept = self.crops.point_batch()
        self.grids = sna.voxelize_batch(self.batch, GRID)
        self.B = len(self.kept)
        torch.manual_seed(1)
        self.pred = torch.rand((self.B, 1) + (GRID[2], GRID[0], GRID[1]), dtype=torch.float32, device=dev)
        tile_of = np.full(self.K, -1, dtype=np.int32)
        tile_of[self.kept] = np.arange(self.B, dtype=np.int32)
        self.tile_of = torch.from_numpy(tile_of).to(dev)
        self.src = self.crops.src_rows()
        self.rows = int(self.src.numel())
        self.out = torch.empty((1, self.n), dtype=torch.float32, device=dev)
        self.cover = torch.empty((self.n,), dtype=torch.int32, device=dev)
        self.ws = torch.empty(_hip.crops_ws_bytes(self.n, self.K) // 8, dtype=torch.int64, device=dev)
        self.offsets = torch.empty(self.K + 1, dtype=torch.int64, device=dev)

    def merge(self, rule, cover):
        _hip.scan_merge(self.pred, self.grids.desc, self.pts, self.regions, self.kinds, self.tile_of, rule, 0.0, self.out,
                        self.cover if cover else None)

    def gather(self):
        return _hip.gather_points(self.pred, self.batch.pts[:self.batch.total_points], self.batch.offsets, self.grids.desc, 0.0)

    def parent(self):
        return sna.merge_to_scan(self.gather()[0], self.src, self.n, 0.0)

    def yardstick(self):
        _hip.crop_count(self.pts, self.regions, self.kinds, self.ws, self.offsets)
        self.gather()

    def variants(self):
        v = {}
        for name, rule in RULES:
            for cover in (False, True):
                v[f"merge {name}{' + cover' if cover else ''}"] = (lambda r=rule, c=cover: self.merge(r, c))
        v["parent: gather_points + merge_to_scan"] = self.parent
        v["yardstick: crop_count + gather_points"] = self.yardstick
        return v


def run_case(case, rounds, iters):
    case.merge(_hip.SN_MERGE_MAX, True)
    assert torch.equal(case.out[0], case.parent()), "rule max differs from gather_points + merge_to_scan"
    variants = case.variants()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        case.merge(_hip.SN_MERGE_INTERIOR, True)
    variants["merge interior + cover, graph replay"] = graph.replay
    for fn in variants.values():       # warm-up: every kernel loaded, every allocation cached
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            times[k].append(once(fn, iters))
    yard = statistics.median(times["yardstick: crop_count + gather_points"])
    mark = ALLOWANCE * yard
    rows = []
    for k, t in times.items():
        med = statistics.median(t)
        row = {"what": k, "median_us": round(med, 1), "min_us": round(min(t), 1), "max_us": round(max(t), 1)}
        if k.startswith("merge"):
            row["verdict"] = "INSIDE" if med <= mark else "OUTSIDE"
            row["over_yardstick"] = round(med / yard, 3)
        rows.append(row)
        print(f"  {k:44s} {med:10.1f} us  [{min(t):.1f} .. {max(t):.1f}]  {row.get('verdict', '')}", flush=True)
    del graph
    return {"case": case.name, "K": case.K, "tiles": case.B, "rows_cropped": case.rows, "mark_us": round(mark, 1),
            "bytes_read_per_call": case.n * 24, "rows": rows}


def kernel_stats(path):
    keep = ("scan_merge", "crop_count", "crop_prefix", "crop_offsets", "gather_points")
    with open(path, newline="") as f:
        return [r for r in csv.DictReader(f) if any(k in r.get("Name", "") for k in keep)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="scan_merge_bench.json")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--trace", action="store_true", help="run every kernel a few times on the 128-box set and exit")
    ap.add_argument("--kernel-stats", default=None, help="kernel_stats csv of a rocprofv3 --kernel-trace --stats run of --trace")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("scan_merge_bench needs a HIP device (there is no CPU path)")
    if args.rounds < 5:
        sys.exit("at least 5 rounds")
    dev = torch.device("cuda:0")
    xyz, _, towers = synthetic_scan(args.points)
    pts = torch.from_numpy(xyz).to(dev)
    sets = region_sets(xyz, towers)
    if args.trace:
        case = Case(*sets[1][:1], pts, *sets[1][1:])
        for _ in range(5):
            for _, rule in RULES:
                case.merge(rule, True)
            case.yardstick()
            case.parent()
        torch.cuda.synchronize()
        return
    res = {"device": torch.cuda.get_device_name(dev), "points": int(pts.shape[0]), "grid": list(GRID), "dtype": "float32",
           "rounds": args.rounds, "iters_per_round": args.iters, "allowance": ALLOWANCE, "cases": []}
    for name, regions, kinds in sets:
        print(name, flush=True)
        case = Case(name, pts, regions, kinds)
        res["cases"].append(run_case(case, args.rounds, args.iters))
        del case
        torch.cuda.empty_cache()
    if args.kernel_stats:
        res["kernel_trace"] = {"set": sets[1][0], "rows": kernel_stats(args.kernel_stats)}
    else:
        res["kernel_trace"] = "not measured"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
