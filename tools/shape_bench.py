#!/usr/bin/env python3
"""K22 neighbourhood shapes on tools/knn_bench.py's two inputs at the radii that tool picked: (a) the 10^6 tower points of
the synthetic scan as one tile at 0.61 m and (b) the C2 batch (32 tiles x 10^5 points) at 0.91 m.  Timed between HIP events
around replayed hipGraphs after a warm-up of every graph, the repeats alternating between the graphs: each launch as the
difference of two prefixes 1..j of the call (sn_shape_points_launches), the whole call eager and replayed, and the shape
launch alone.  After the timing the outputs of a replay are compared bit for bit with the eager call's.
Yardstick, measured in the same run: K21's search launch at k = 1 on the same points and the same cells, replayed alone and
alternating with the shape launch -- the same loads and candidate tests, one list slot where K22 keeps ten integers and then
solves a 3x3.  The mark is 1.25 x the yardstick: INSIDE or OUTSIDE per input.
Baselines: on the device, what a user has without K22 -- sn_knn_points with index at k = 16, a gather, the covariance and
torch.linalg.eigh, on a part of the rows and scaled (capped at 16 neighbours: not the same result); on the host, the part
copied down, sklearn's radius_neighbors, numpy's covariance and np.linalg.eigh, scaled.  The bench checks K22's eigenvalues
against the host's on that part (the quantum is 2^-16 of the radius).  Writes one JSON file.
    python tools/shape_bench.py --out profiles/shape_bench.json [--iters 5] [--repeats 5]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/shape_bench.py --trace   # the program for a kernel trace: input
                                                     # (a), eager calls of sna.shape_features and of K21 at k = 1"""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
import scene_net_amd as sna  # noqa: E402
from scene_net_amd import _hip  # noqa: E402
from scene_net_amd.synthetic import synthetic_tile  # noqa: E402
from crops_bench import synthetic_scan  # noqa: E402
from knn_bench import alternating_us, graph_of, pairs_27  # noqa: E402

MAX_CELLS, MARK = 1 << 18, 1.25
RADIUS_A, RADIUS_B = 0.2 * 1.25 ** 5, 0.05 * 1.25 ** 13          # profiles/knn_bench.json: 0.6103515625, 0.9094947...
LAUNCHES = ("zero", "cells", "prefix", "scatter", "shape")


def case(name, tiles, dev, iters, repeats, radius):
    B, total = len(tiles), sum(len(t) for t in tiles)
    batch = sna.PointBatch.from_tiles(tiles, device=dev)
    lo_np = np.stack([t.min(axis=0) for t in tiles])
    lo = torch.from_numpy(lo_np).to(dev).reshape(-1)
    extent = [float(v) for v in np.max([t.max(axis=0) - t.min(axis=0) for t in tiles], axis=0)]
    dims, side = _hip.dbscan_cell_grid([0.0, 0.0, 0.0] + extent, radius, MAX_CELLS // B)
    mult = int(round(side / (radius * (1.0 + 2.0 ** -20))))
    cells = dims[0] * dims[1] * dims[2]
    pairs = pairs_27(tiles, lo_np, dims, side)
    res = {"case": name, "points": total, "tiles": B, "radius": radius, "grid_per_tile": list(dims), "mult": mult,
           "cell_side": side, "candidate_tests_27_cells": pairs}
    print(f"{name}: {total} points in {B} tiles, radius {radius:.4f}, grid {dims} x {B}, {pairs:.3e} candidate tests", flush=True)

    ws = torch.empty(_hip.shape_ws_bytes(total, B, cells) // 8, dtype=torch.int64, device=dev)
    count = torch.empty(total, dtype=torch.int32, device=dev)
    moments = torch.empty((total, 9), dtype=torch.int64, device=dev)
    eig, normal, axis = (torch.empty((total, 3), dtype=torch.float64, device=dev) for _ in range(3))
    feat = torch.empty((total, _hip.SN_SHAPE_NFEAT), dtype=torch.float64, device=dev)

    def shape(launches=None):
        _hip.shape_points(batch.pts, batch.offsets, radius, 3, lo, dims, mult, ws, count, moments, eig, normal, axis, feat,
                          launches=launches)

    kws = torch.empty(_hip.knn_ws_bytes(total, B, cells) // 8, dtype=torch.int64, device=dev)
    d2 = torch.empty((total, 1), dtype=torch.float64, device=dev)
    found = torch.empty(total, dtype=torch.int32, device=dev)

    def knn(launches=None):
        _hip.knn_points(batch.pts, batch.offsets, radius, 1, lo, dims, mult, kws, d2, found, None, None, launches=launches)
    knn()
    gc.collect()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        shape()
    torch.cuda.synchronize()
    eager_us = (time.perf_counter() - t0) * 1e6 / iters
    outs = (count, moments, eig, normal, axis, feat)
    want = [t.clone() for t in outs]
    n = _hip.SN_SHAPE_LAUNCHES
    graphs = {f"prefix_{j}": graph_of(lambda j=j: shape((1, j))) for j in range(1, n + 1)}
    graphs["whole"] = graph_of(shape)
    graphs["shape_alone"] = graph_of(lambda: shape((n, n)))
    graphs["knn_k1_search_alone"] = graph_of(lambda: knn((4, 4)))
    med, raw = alternating_us(graphs, iters, repeats)
    graphs["whole"].replay()
    torch.cuda.synchronize()
    same = all(torch.equal(a.view(torch.int64) if a.dtype == torch.float64 else a,
                           b.view(torch.int64) if b.dtype == torch.float64 else b) for a, b in zip(outs, want))
    assert same, "the replayed graphs left other bits than the eager call"
    prefix = [0.0] + [med[f"prefix_{j}"] for j in range(1, n + 1)]
    ratio = med["shape_alone"] / med["knn_k1_search_alone"]
    live = count >= 3
    res.update({"launch_us_by_differences": {nm: round(prefix[j] - prefix[j - 1], 2) for j, nm in enumerate(LAUNCHES, start=1)},
                "whole_call_eager_us": round(eager_us, 2), "whole_call_replayed_us": round(med["whole"], 2),
                "shape_alone_us": round(med["shape_alone"], 2), "knn_k1_search_alone_us": round(med["knn_k1_search_alone"], 2),
                "shape_over_knn_k1_search": round(ratio, 3), "mark": MARK, "verdict": "INSIDE" if ratio <= MARK else "OUTSIDE",
                "replays_equal_eager_bits": same, "candidate_tests_per_s_shape": round(pairs / (med["shape_alone"] * 1e-6), 0),
                "rows_with_3_members": int(live.sum()), "mean_members": round(float(count.double().mean()), 2),
                "max_members": int(count.max()),
                "repeats_us": {nm: raw[nm] for nm in ("shape_alone", "knn_k1_search_alone", "whole")}})
    print(f"  shape {res['shape_alone_us']} us, K21 k = 1 search {res['knn_k1_search_alone_us']} us, ratio "
          f"{res['shape_over_knn_k1_search']} {res['verdict']}; whole eager {res['whole_call_eager_us']} us, replayed "
          f"{res['whole_call_replayed_us']} us; launches {res['launch_us_by_differences']}", flush=True)
    del graphs
    return res, batch, lo, extent, eig.clone(), count.clone()


def device_baseline(res, batch, lo, extent, radius, part, scale, iters):
    """index at k = 16 (the whole batch: the search cannot be cut), then gather + covariance + torch.linalg.eigh on the first
    `part` rows, scaled"""
    k = 16
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        nb = sna.knn_distances(batch, k, radius, want_index=True, want_mean=False, lo=lo.reshape(-1, 3), extent=extent,
                               max_cells=MAX_CELLS)
    torch.cuda.synchronize()
    knn_ms = (time.perf_counter() - t0) * 1e3 / iters
    idx, pts = nb.index[:part], batch.pts

    def rest():
        ok = idx >= 0
        q = pts[idx.clamp(min=0)] - pts[:part, None, :]
        q = torch.where(ok[:, :, None], q, torch.zeros_like(q))
        n = (ok.sum(dim=1) + 1).double()[:, None]
        mean = q.sum(dim=1) / n
        cov = torch.einsum("nka,nkb->nab", q, q) / n[:, :, None] - mean[:, :, None] * mean[:, None, :]
        return torch.linalg.eigh(cov)
    rest()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        rest()
    torch.cuda.synchronize()
    rest_ms = (time.perf_counter() - t0) * 1e3 / iters
    res["device_baseline"] = {"knn_k16_index_ms": round(knn_ms, 2), "gather_cov_eigh_ms_part": round(rest_ms, 2),
                              "part_points": part, "scale": scale, "total_ms_scaled": round(knn_ms + rest_ms * scale, 1),
                              "capped_at_neighbours": k}
    res["device_baseline_over_whole_call_replayed"] = round((knn_ms + rest_ms * scale) * 1e3 / res["whole_call_replayed_us"], 1)
    print(f"  device baseline: knn k = 16 {knn_ms:.1f} ms + gather/cov/eigh {rest_ms:.1f} ms x {scale}", flush=True)


def host_baseline(res, batch, radius, part, scale, eig, count):
    """the first `part` rows (a part no neighbour of which lies outside it) copied down; sklearn's radius_neighbors, numpy's
    covariance and eigh, scaled; K22's eigenvalues checked against it"""
    from sklearn.neighbors import NearestNeighbors
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    P = batch.pts[:part].cpu().numpy()
    d2h_ms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    ind = NearestNeighbors(radius=radius, algorithm="kd_tree").fit(P).radius_neighbors(P, return_distance=False)
    cov = np.zeros((part, 3, 3))
    for i, nb in enumerate(ind):
        q = P[nb] - P[i]
        m = q.mean(axis=0)
        cov[i] = q.T @ q / len(nb) - np.outer(m, m)
    w = np.linalg.eigvalsh(cov)
    host_ms = (time.perf_counter() - t0) * 1e3
    live = (count[:part] >= 3).cpu().numpy() & (w[:, 2] > 0)
    got = eig[:part].cpu().numpy()
    members_equal = float((np.array([len(nb) for nb in ind]) == count[:part].cpu().numpy()).mean())
    close = bool(np.allclose(got[live], w[live], rtol=1e-3, atol=1e-3 * float(w[live, 2].max()))) if live.any() else True
    res["host"] = {"d2h_ms": round(d2h_ms, 2), "sklearn_numpy_ms_part": round(host_ms, 1), "part_points": part, "scale": scale,
                   "total_ms_scaled": round(d2h_ms + host_ms * scale, 1), "eigenvalues_close_on_that_part": close,
                   "share_of_rows_with_equal_member_count": round(members_equal, 6)}
    res["host_over_whole_call_replayed"] = round((d2h_ms + host_ms * scale) * 1e3 / res["whole_call_replayed_us"], 1)
    print(f"  host: d2h {d2h_ms:.1f} ms + sklearn/numpy {host_ms:.0f} ms x {scale}; eigenvalues close: {close}; equal member "
          f"counts {members_equal:.6f}", flush=True)
    assert close


def trace_program(dev, points, calls=3):
    """what a kernel trace is taken of: the whole call and K21's at k = 1 on input (a), eager, `calls` times each"""
    pts, labels, _ = synthetic_scan(points)
    towers = np.ascontiguousarray(pts[labels == 15.0])
    batch = sna.PointBatch.from_tiles([towers], device=dev)
    lo = torch.from_numpy(towers.min(axis=0)[None]).to(dev)
    extent = [float(v) for v in towers.max(axis=0) - towers.min(axis=0)]
    for _ in range(calls):
        sna.shape_features(batch, RADIUS_A, lo=lo, extent=extent, max_cells=MAX_CELLS)
        sna.knn_distances(batch, 1, RADIUS_A, lo=lo, extent=extent, max_cells=MAX_CELLS)
        torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="shape_bench.json")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--points", type=int, default=10_000_000, help="points of the synthetic scan (its towers are 10 %%)")
    ap.add_argument("--tiles", type=int, default=32)
    ap.add_argument("--tile-points", type=int, default=100_000)
    ap.add_argument("--trace", action="store_true", help="run the program a rocprofv3 kernel trace is taken of, and nothing else")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("shape_bench needs a HIP device (there is no CPU path)")
    dev = torch.device("cuda:0")
    if args.trace:
        return trace_program(dev, args.points)
    res = {"device": torch.cuda.get_device_name(dev), "max_cells": MAX_CELLS, "sweeps": _hip.SN_SHAPE_SWEEPS, "cases": []}

    pts, labels, _ = synthetic_scan(args.points)
    towers = np.ascontiguousarray(pts[labels == 15.0])
    first_tower = int((labels[:args.points // 128] == 15.0).sum())      # the scan's tiles follow each other: tile 0's tower
    del pts, labels
    c, batch, lo, extent, eig, count = case(f"the {len(towers)} tower points of the synthetic scan, one tile", [towers], dev,
                                            args.iters, args.repeats, RADIUS_A)
    device_baseline(c, batch, lo, extent, RADIUS_A, first_tower, 128, args.iters)
    host_baseline(c, batch, RADIUS_A, first_tower, 128, eig, count)
    res["cases"].append(c)
    print(json.dumps(c), flush=True)
    del batch, towers, eig, count

    tiles = [synthetic_tile(t, args.tile_points)[0] for t in range(args.tiles)]
    c, batch, lo, extent, eig, count = case(f"C2 batch, {args.tiles} tiles x {args.tile_points} points", tiles, dev, args.iters,
                                            args.repeats, RADIUS_B)
    res["cases"].append(c)
    print(json.dumps(c), flush=True)

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
