#!/usr/bin/env python3
"""K21 nearest neighbours on (a) the 10^6 tower points of tools/dbscan_bench.py's synthetic scan as one tile and (b) the C2
batch (32 tiles x 10^5 points, all at the same origin) as a CSR batch, for k = 1, 8, 16 at a radius the tool picks so that
n_full / n_valid >= 0.9 at k = 8 (printed).  Timed between HIP events around replayed hipGraphs after a warm-up of every
graph, the repeats alternating between the graphs: each launch as the difference of two prefixes 1..j of the call
(sn_knn_points_launches), the whole call (search + statistics) eager and replayed, remove_outliers end to end replayed.
Candidate tests: the rows a point meets in the 27 cells around its own, summed over the points (counted on the host on the
same grid).  After the timing the outputs of a replay are compared bit for bit with the eager call's.
Yardstick: K10's own candidate walk -- launch 4 of sn_dbscan_points_launches with min_points beyond any neighbourhood (no
early exit) on the same points, the same cell side and eps = radius: the same loads and the same distance test, a counter
where K21 keeps a list.  Both launches are replayed alone (their launches 1..3 have run on the workspace), alternating.
The mark is 1.25 x the yardstick: INSIDE or OUTSIDE per input and k.  For (b) K10 has no tiles: the tiles are laid side by
side 64 m apart, which leaves every point's candidates what they are.
Host baseline: the points copied down and sklearn.neighbors.NearestNeighbors(algorithm='kd_tree').kneighbors on one tower /
one tile, scaled to all.  The bench checks what it times against sklearn on that part.  Writes one JSON file.
    python tools/knn_bench.py --out profiles/knn_bench.json [--iters 5] [--repeats 5]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/knn_bench.py --trace     # the program for a kernel trace: input
                                                     # (a) at the radius of the JSON, eager calls at k = 1, 8, 16 and K10's walk"""
import argparse
import gc
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import scene_net_amd as sna  # noqa: E402
from scene_net_amd import _hip  # noqa: E402
from scene_net_amd.synthetic import synthetic_tile  # noqa: E402
from crops_bench import synthetic_scan  # noqa: E402

KS, MAX_CELLS, FULL_SHARE, MARK = (1, 8, 16), 1 << 18, 0.9, 1.25
LAUNCHES = ("cells", "prefix", "scatter", "search")
K10_UNION_TESTS_PER_S = 1.3e11          # DESIGN section 7 K10, its union launch


def graph_of(fn):
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g


def alternating_us(graphs, iters, repeats):
    """{name: median us per replay}: every graph warmed up, then `repeats` rounds that time each graph in turn"""
    for g in graphs.values():
        for _ in range(3):
            g.replay()
    torch.cuda.synchronize()
    times = {name: [] for name in graphs}
    for _ in range(repeats):
        for name, g in graphs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                g.replay()
            b.record()
            torch.cuda.synchronize()
            times[name].append(a.elapsed_time(b) * 1e3 / iters)
    return {name: statistics.median(v) for name, v in times.items()}, {name: [round(x, 2) for x in v] for name, v in times.items()}


def pairs_27(tiles, lo, dims, side):
    """sum over the points of the rows in the 27 cells around their own, tile by tile on the grid the entry lays out"""
    total = 0
    for P, l in zip(tiles, lo):
        c = [np.clip(np.floor((P[:, a] - l[a]) * (1.0 / side)), 0, dims[a] - 1).astype(np.int64) for a in range(3)]
        pop = np.zeros(tuple(d + 2 for d in dims), dtype=np.int64)
        np.add.at(pop, (c[0] + 1, c[1] + 1, c[2] + 1), 1)
        around = sum(pop[1 + i:pop.shape[0] - 1 + i, 1 + j:pop.shape[1] - 1 + j, 1 + k:pop.shape[2] - 1 + k]
                     for i in (-1, 0, 1) for j in (-1, 0, 1) for k in (-1, 0, 1))
        total += int((pop[1:-1, 1:-1, 1:-1] * around).sum())
    return total


def pick_radius(batch, lo, extent, start):
    """the first radius of start * 1.25^j with n_full / n_valid >= FULL_SHARE at k = 8 over the whole batch"""
    r = start
    for _ in range(40):
        st = sna.knn_distances(batch, 8, r, lo=lo, extent=extent, max_cells=MAX_CELLS).stats.sum(dim=0).cpu().tolist()
        share = st[1] / max(st[0], 1.0)
        print(f"  radius {r:.4f}: n_full / n_valid = {share:.4f}", flush=True)
        if share >= FULL_SHARE:
            return r, share
        r *= 1.25
    sys.exit("no radius found")


def case(name, tiles, dev, iters, repeats, start_radius, k10_shift):
    sizes = [len(t) for t in tiles]
    B, total = len(tiles), sum(sizes)
    batch = sna.PointBatch.from_tiles(tiles, device=dev)
    lo_np = np.stack([t.min(axis=0) for t in tiles])
    lo = torch.from_numpy(lo_np).to(dev)
    extent = [float(v) for v in np.max([t.max(axis=0) - t.min(axis=0) for t in tiles], axis=0)]
    print(f"{name}: {total} points in {B} tiles, extent {extent}", flush=True)
    radius, share = pick_radius(batch, lo, extent, start_radius)
    per_tile = MAX_CELLS // B
    dims, side = _hip.dbscan_cell_grid([0.0, 0.0, 0.0] + extent, radius, per_tile)
    mult = int(round(side / (radius * (1.0 + 2.0 ** -20))))
    pairs = pairs_27(tiles, lo_np, dims, side)
    res = {"case": name, "points": total, "tiles": B, "radius": radius, "n_full_over_n_valid_at_k8": round(share, 4),
           "grid_per_tile": list(dims), "mult": mult, "cell_side": side, "candidate_tests_27_cells": pairs, "k": {}}
    print(f"  radius {radius:.4f} (share {share:.4f}), grid {dims} x {B}, mult {mult}, {pairs:.3e} candidate tests", flush=True)

    # K10 on the same points: tiles side by side, one grid of the same cell side
    shifted = np.concatenate([t + np.array([k10_shift * b, 0.0, 0.0]) for b, t in enumerate(tiles)])
    d_shift = torch.from_numpy(shifted).to(dev)
    bounds = np.concatenate([shifted.min(axis=0), shifted.max(axis=0)]).tolist()
    # the cell budget under which K10 lays cells of the same side (else of the nearest side: recorded)
    k10_cells = min((MAX_CELLS << j for j in range(5)), key=lambda c: abs(_hip.dbscan_cell_grid(bounds, radius, c)[1] - side))
    k10_dims, k10_side = _hip.dbscan_cell_grid(bounds, radius, k10_cells)
    res["k10"] = {"grid": list(k10_dims), "cell_side": k10_side, "same_cell_side": bool(k10_side == side)}
    k10_ws = torch.empty(_hip.dbscan_ws_bytes(total, k10_dims[0] * k10_dims[1] * k10_dims[2]) // 8, dtype=torch.int64, device=dev)
    cluster = torch.empty(total, dtype=torch.int32, device=dev)
    n_clusters, status = torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)

    def k10(launches):
        _hip.dbscan_points(d_shift, None, None, bounds, radius, 1 << 30, k10_cells, 0, k10_ws, cluster, n_clusters, None, status,
                           launches=launches)
    k10((1, 4))
    torch.cuda.synchronize()
    res["k10"]["pairs_27_cells"] = pairs_27([shifted], [bounds[:3]], k10_dims, k10_side)

    ws = torch.empty(_hip.knn_ws_bytes(total, B, dims[0] * dims[1] * dims[2]) // 8, dtype=torch.int64, device=dev)
    found = torch.empty(total, dtype=torch.int32, device=dev)
    mean = torch.empty(total, dtype=torch.float64, device=dev)
    stats = torch.empty((B, _hip.SN_KNN_NSTAT), dtype=torch.float64, device=dev)
    for k in KS:
        d2 = torch.empty((total, k), dtype=torch.float64, device=dev)

        def knn(launches=None, k=k, d2=d2):
            _hip.knn_points(batch.pts, batch.offsets, radius, k, lo, dims, mult, ws, d2, found, mean, None, launches=launches)

        def whole(k=k):
            knn()
            _hip.knn_tile_stats(mean, found, batch.offsets, k, ws, stats)
        gc.collect()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            whole()
        torch.cuda.synchronize()
        eager_us = (time.perf_counter() - t0) * 1e6 / iters
        want = (d2.clone(), found.clone(), stats.clone())
        graphs = {f"prefix_{j}": graph_of(lambda j=j: knn((1, j))) for j in range(1, 5)}
        graphs["whole"] = graph_of(whole)
        graphs["knn_search_alone"] = graph_of(lambda: knn((4, 4)))
        graphs["k10_core_alone"] = graph_of(lambda: k10((4, 4)))
        med, raw = alternating_us(graphs, iters, repeats)
        graphs["whole"].replay()
        torch.cuda.synchronize()
        same = bool(torch.equal(d2, want[0]) and torch.equal(found, want[1]) and torch.equal(stats, want[2]))
        assert same, "the replayed graphs left other bits than the eager call"
        prefix = [0.0] + [med[f"prefix_{j}"] for j in range(1, 5)]
        per = {n: round(prefix[j] - prefix[j - 1], 2) for j, n in enumerate(LAUNCHES, start=1)}
        ratio = med["knn_search_alone"] / med["k10_core_alone"]
        out = {"launch_us_by_differences": per, "whole_call_eager_us": round(eager_us, 2),
               "whole_call_replayed_us": round(med["whole"], 2), "search_alone_us": round(med["knn_search_alone"], 2),
               "k10_core_walk_alone_us": round(med["k10_core_alone"], 2), "search_over_k10_walk": round(ratio, 3),
               "replays_equal_eager_bits": same, "mark": MARK, "verdict": "INSIDE" if ratio <= MARK else "OUTSIDE",
               "candidate_tests_per_s_search": round(pairs / (med["knn_search_alone"] * 1e-6), 0),
               "k10_tests_per_s_core_walk": round(res["k10"]["pairs_27_cells"] / (med["k10_core_alone"] * 1e-6), 0),
               "k10_union_tests_per_s_quoted": K10_UNION_TESTS_PER_S,
               "repeats_us": {n: raw[n] for n in ("knn_search_alone", "k10_core_alone", "whole")}}
        res["k"][str(k)] = out
        print(f"  k = {k}: search {out['search_alone_us']} us, K10 walk {out['k10_core_walk_alone_us']} us, ratio "
              f"{out['search_over_k10_walk']} {out['verdict']}; whole eager {out['whole_call_eager_us']} us, replayed "
              f"{out['whole_call_replayed_us']} us; {out['candidate_tests_per_s_search']:.3e} tests/s; launches {per}", flush=True)
        del graphs

    ro = graph_of(lambda: sna.remove_outliers(batch, k=8, radius=radius, capacity=total, lo=lo, extent=extent,
                                              max_cells=MAX_CELLS))
    med, _ = alternating_us({"remove_outliers": ro}, iters, repeats)
    res["remove_outliers_k8_replayed_us"] = round(med["remove_outliers"], 2)
    kept = sna.remove_outliers(batch, k=8, radius=radius, lo=lo, extent=extent, max_cells=MAX_CELLS)
    res["remove_outliers_kept"] = int(kept.batch.offsets[-1])
    print(f"  remove_outliers (k = 8, statistical, 2 sigma): {res['remove_outliers_k8_replayed_us']} us replayed, kept "
          f"{res['remove_outliers_kept']} of {total}", flush=True)

    return res, batch, lo, extent, radius


def host_baseline(res, batch, lo, extent, radius, n0, scale):
    """the points copied down; sklearn's kd-tree at k = 8 on the first n0 rows (a part no neighbour of which lies outside
    it), scaled to all; the device's distances checked against it on the rows with 8 neighbours"""
    from sklearn.neighbors import NearestNeighbors
    k = 8
    nb = sna.knn_distances(batch, k, radius, lo=lo, extent=extent, max_cells=MAX_CELLS)
    batch_part_d2, batch_part_found = nb.d2[:n0].cpu().numpy(), nb.found[:n0].cpu().numpy()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    part = batch.pts.cpu().numpy()[:n0]
    d2h_ms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    dist, _ = NearestNeighbors(n_neighbors=k + 1, algorithm="kd_tree").fit(part).kneighbors(part)
    sk_ms = (time.perf_counter() - t0) * 1e3
    full = batch_part_found >= k
    same = bool(np.allclose(dist[full, 1:], np.sqrt(batch_part_d2[full]), rtol=1e-12, atol=0.0))
    res["host"] = {"d2h_ms": round(d2h_ms, 2), "sklearn_kd_tree_k8_ms_part": round(sk_ms, 1), "part_points": len(part),
                   "scale": scale, "sklearn_kd_tree_k8_ms_scaled": round(sk_ms * scale, 1),
                   "distances_equal_on_full_rows_of_that_part": same}
    res["host_over_whole_call_replayed_k8"] = round((d2h_ms + sk_ms * scale) * 1e3 / res["k"]["8"]["whole_call_replayed_us"], 1)
    print(f"  host: d2h {d2h_ms:.1f} ms + sklearn {sk_ms:.0f} ms x {scale} ; equal on the part: {same}", flush=True)
    assert same


def trace_program(dev, points, radius, calls=3):
    """what a kernel trace is taken of: the whole call at every k and K10's launches 1..4, eager, `calls` times each"""
    pts, labels, _ = synthetic_scan(points)
    towers = np.ascontiguousarray(pts[labels == 15.0])
    batch = sna.PointBatch.from_tiles([towers], device=dev)
    lo = torch.from_numpy(towers.min(axis=0)[None]).to(dev)
    extent = [float(v) for v in towers.max(axis=0) - towers.min(axis=0)]
    bounds = np.concatenate([towers.min(axis=0), towers.max(axis=0)]).tolist()
    dims, _ = _hip.dbscan_cell_grid(bounds, radius, MAX_CELLS)
    total = len(towers)
    k10_ws = torch.empty(_hip.dbscan_ws_bytes(total, dims[0] * dims[1] * dims[2]) // 8, dtype=torch.int64, device=dev)
    cluster = torch.empty(total, dtype=torch.int32, device=dev)
    n_clusters, status = torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    for _ in range(calls):
        for k in KS:
            sna.knn_distances(batch, k, radius, lo=lo, extent=extent, max_cells=MAX_CELLS)
        _hip.dbscan_points(batch.pts, None, None, bounds, radius, 1 << 30, MAX_CELLS, 0, k10_ws, cluster, n_clusters, None, status,
                           launches=(1, 4))
        torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="knn_bench.json")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--points", type=int, default=10_000_000, help="points of the synthetic scan (its towers are 10 %%)")
    ap.add_argument("--tiles", type=int, default=32)
    ap.add_argument("--tile-points", type=int, default=100_000)
    ap.add_argument("--trace", action="store_true", help="run the program a rocprofv3 kernel trace is taken of, and nothing else")
    ap.add_argument("--trace-radius", type=float, default=0.6103515625, help="input (a)'s radius in profiles/knn_bench.json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("knn_bench needs a HIP device (there is no CPU path)")
    dev = torch.device("cuda:0")
    if args.trace:
        return trace_program(dev, args.points, args.trace_radius)
    res = {"device": torch.cuda.get_device_name(dev), "max_cells": MAX_CELLS, "full_share": FULL_SHARE, "cases": []}

    pts, labels, _ = synthetic_scan(args.points)
    towers = np.ascontiguousarray(pts[labels == 15.0])
    first_tower = int((labels[:args.points // 128] == 15.0).sum())      # the scan's tiles follow each other: tile 0's tower
    del pts, labels
    c, batch, lo, extent, radius = case(f"the {len(towers)} tower points of the synthetic scan, one tile", [towers], dev,
                                        args.iters, args.repeats, 0.2, 0.0)
    host_baseline(c, batch, lo, extent, radius, first_tower, 128)
    res["cases"].append(c)
    print(json.dumps(c), flush=True)
    del batch, towers

    tiles = [synthetic_tile(t, args.tile_points)[0] for t in range(args.tiles)]
    c, batch, lo, extent, radius = case(f"C2 batch, {args.tiles} tiles x {args.tile_points} points", tiles, dev, args.iters,
                                        args.repeats, 0.05, 64.0)
    host_baseline(c, batch, lo, extent, radius, len(tiles[0]), args.tiles)
    res["cases"].append(c)
    print(json.dumps(c), flush=True)

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
