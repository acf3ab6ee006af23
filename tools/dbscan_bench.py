#!/usr/bin/env python3
"""K10 point DBSCAN on the synthetic scan of tools/crops_bench.py (10^7 points, 128 tiles, the tower points 10 % of each)
with eps = 10, min_points = 300, and on one dense tower of 2 * 10^5 points -- what the clustering costs without the
dense-cell shortcut.  Timed between HIP events after a warm-up: sn_points_select, sn_dbscan_points as a whole, each of its
launches as the difference of two prefixes 1..k of the call (sn_dbscan_points_launches), and select + cluster captured
into a hipGraph and replayed.  Pairs: the rows a point meets in the 27 cells around its own, summed over the points
(counted on the host from the same grid); launch 5 takes the distance of a pair once, by its larger position, so its
distance tests are pairs / 2 where every point is core.  Baseline: the tower points copied to the host and
sklearn.cluster.DBSCAN(algorithm='kd_tree') on the towers of a few tiles, scaled to all (its neighbour lists for the
whole scan do not fit a host's memory); on the dense tower sklearn runs on a subsample and is scaled by (n / n_sub)^2.
The bench checks what it times: the cluster count, and the labels of the tiles sklearn saw.  Writes one JSON file.
    python tools/dbscan_bench.py --out profiles/dbscan_bench.json [--iters 5]"""
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
from crops_bench import synthetic_scan  # noqa: E402

EPS, MIN_POINTS, MAX_CLUSTERS, MAX_CELLS = 10.0, 300, 256, 1 << 18
LAUNCHES = ("cells", "prefix", "scatter", "core", "union", "flatten", "rank", "finish")


def timed(fn, iters, spin_ms=100.0):
    """ms per call by events over `iters` calls, after ~spin_ms of the same work and a synchronise."""
    gc.collect()
    t0 = time.perf_counter()
    while True:
        fn()
        torch.cuda.synchronize()
        if (time.perf_counter() - t0) * 1e3 >= spin_ms:
            break
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def pairs_27(P, bounds, eps):
    """sum over the points of the rows in the 27 cells around their own, on the grid the entry lays out"""
    dims, side = _hip.dbscan_cell_grid(bounds, eps, MAX_CELLS)
    c = [np.clip(np.floor((P[:, a] - bounds[a]) * (1.0 / side)), 0, dims[a] - 1).astype(np.int64) for a in range(3)]
    pop = np.zeros(tuple(d + 2 for d in dims), dtype=np.int64)
    np.add.at(pop, (c[0] + 1, c[1] + 1, c[2] + 1), 1)
    around = sum(pop[1 + i:pop.shape[0] - 1 + i, 1 + j:pop.shape[1] - 1 + j, 1 + k:pop.shape[2] - 1 + k]
                 for i in (-1, 0, 1) for j in (-1, 0, 1) for k in (-1, 0, 1))
    return int((pop[1:-1, 1:-1, 1:-1] * around).sum()), list(dims), int((pop > 0).sum())


def sklearn_ms(P):
    from sklearn.cluster import DBSCAN
    t0 = time.perf_counter()
    labels = DBSCAN(eps=EPS, min_samples=MIN_POINTS, algorithm="kd_tree").fit(P).labels_
    return (time.perf_counter() - t0) * 1e3, labels


def cluster_case(name, pts, labels, dev, iters):
    """select, cluster, per launch, captured replay of one scan (numpy in, dict out)"""
    d_pts = torch.from_numpy(pts).to(dev)
    d_lab = torch.from_numpy(labels).to(dev)
    keep = torch.tensor([15.0], dtype=torch.float64, device=dev)
    n = len(pts)
    found = sna.cluster_points(d_pts, EPS, MIN_POINTS, labels=d_lab, keep=keep, max_clusters=MAX_CLUSTERS, max_cells=MAX_CELLS)
    m, K = int(found.n_sel), int(found.n_clusters)
    sel_ws = torch.empty(_hip.points_select_ws_bytes(n) // 8, dtype=torch.int64, device=dev)
    sel = torch.empty(m, dtype=torch.int64, device=dev)
    n_sel, bbox = torch.zeros(1, dtype=torch.int64, device=dev), torch.zeros(6, dtype=torch.float64, device=dev)
    _hip.points_select(d_pts, d_lab, keep, sel_ws, sel, n_sel, bbox)
    bounds = bbox.cpu().tolist()
    assert int(n_sel) == m == int((labels == 15.0).sum())
    pairs, dims, cells_used = pairs_27(pts[labels == 15.0], bounds, EPS)
    ws = torch.empty(_hip.dbscan_ws_bytes(m, dims[0] * dims[1] * dims[2]) // 8, dtype=torch.int64, device=dev)
    cluster = torch.empty(m, dtype=torch.int32, device=dev)
    n_clusters, status = torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    stats = torch.zeros((MAX_CLUSTERS, 3), dtype=torch.int64, device=dev)

    def select():
        _hip.points_select(d_pts, d_lab, keep, sel_ws, sel, n_sel, bbox)

    def entry(launches=None):
        _hip.dbscan_points(d_pts, sel, n_sel, bounds, EPS, MIN_POINTS, MAX_CELLS, MAX_CLUSTERS, ws, cluster, n_clusters, stats,
                           status, launches=launches)
    t0 = time.perf_counter()
    entry()
    torch.cuda.synchronize()
    first_ms = (time.perf_counter() - t0) * 1e3
    print(f"{name}: m = {m}, K = {K}, grid {dims}, first call {first_ms:.1f} ms", flush=True)
    assert int(n_clusters) == K and int(status) == 0 and torch.equal(cluster, found.cluster)
    spin = 100.0 if first_ms < 50 else 0.0
    res = {"case": name, "n": n, "selected": m, "clusters": K, "n_core": int(stats[:, 1].sum()), "grid": dims,
           "cells_used": cells_used, "pairs_27_cells": pairs, "select_us": round(timed(select, max(iters, 10)) * 1e3, 2)}
    whole = timed(entry, iters, spin)
    res["cluster_us"] = round(whole * 1e3, 2)
    print(f"  select {res['select_us']} us, cluster {res['cluster_us']} us", flush=True)
    # per launch: the prefixes 1..k, each from a fresh start (launch 4 resets the parents), and their differences
    prefix = [0.0]
    for k in range(1, len(LAUNCHES) + 1):
        prefix.append(timed(lambda k=k: entry((1, k)), iters, spin))
        print(f"  launches 1..{k}: {prefix[-1] * 1e3:.1f} us", flush=True)
    per = {name_: round((prefix[k] - prefix[k - 1]) * 1e3, 2) for k, name_ in enumerate(LAUNCHES, start=1)}
    res.update({"launch_us": per, "prefix_us": [round(v * 1e3, 2) for v in prefix[1:]], "dominant_launch": max(per, key=per.get)})
    entry()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        select()
        entry()
    res["graph_replay_us"] = round(timed(graph.replay, iters, spin) * 1e3, 2)
    union_s = max(per["union"], 1e-3) * 1e-6
    res["union_distance_tests_per_s_if_all_core"] = round(pairs / 2 / union_s, 0)
    res["pairs_per_s_whole_entry"] = round(pairs / (whole * 1e-3), 0)
    del graph
    return res, found, d_pts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="dbscan_bench.json")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--dense", type=int, default=200_000)
    ap.add_argument("--host-tiles", type=int, default=2, help="tiles whose towers sklearn clusters (scaled to all)")
    ap.add_argument("--dense-sub", type=int, default=10_000, help="points of the dense tower sklearn clusters")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("dbscan_bench needs a HIP device (there is no CPU path)")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(dev), "eps": EPS, "min_points": MIN_POINTS, "max_cells": MAX_CELLS, "cases": []}

    pts, labels, _ = synthetic_scan(args.points)
    c, found, d_pts = cluster_case(f"scan of {args.points} points, 128 towers", pts, labels, dev, args.iters)
    # host baseline: the tower points copied down, sklearn on the towers of the first tiles
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    towers_host = d_pts[found.sel].cpu().numpy()
    d2h_ms = (time.perf_counter() - t0) * 1e3
    per_tile = args.points // 128
    head = int((labels[:per_tile * args.host_tiles] == 15.0).sum())
    sk_ms, sk_labels = sklearn_ms(towers_host[:head])
    same = bool(np.array_equal(found.cluster[:head].cpu().numpy(), sk_labels))
    assert len(set(sk_labels.tolist()) - {-1}) == args.host_tiles and c["clusters"] == 128
    c["host"] = {"d2h_gather_ms": round(d2h_ms, 2), "sklearn_kd_tree_ms_tiles": round(sk_ms, 1), "tiles_timed": args.host_tiles,
                 "sklearn_kd_tree_ms_scaled": round(sk_ms * 128 / args.host_tiles, 1), "labels_equal_on_those_tiles": same}
    c["host_over_select_plus_cluster"] = round((d2h_ms + sk_ms * 128 / args.host_tiles) * 1e3 / (c["select_us"] + c["cluster_us"]), 1)
    res["cases"].append(c)
    print(json.dumps(c), flush=True)
    del found, d_pts

    rng = np.random.default_rng(9)
    dense = np.array([5.44e5, 4.634e6, 1.5e2]) + np.column_stack([rng.normal(15, 1.5, args.dense), rng.normal(15, 1.5, args.dense),
                                                                  rng.uniform(0, 30, args.dense)])
    c, found, d_pts = cluster_case(f"one dense tower of {args.dense} points", dense, np.full(args.dense, 15.0), dev,
                                   max(2, args.iters // 2))
    sub = dense[rng.choice(args.dense, args.dense_sub, replace=False)]
    sk_ms, _ = sklearn_ms(sub)
    c["host"] = {"sklearn_kd_tree_ms_subsample": round(sk_ms, 1), "subsample": args.dense_sub,
                 "sklearn_kd_tree_ms_scaled_quadratically": round(sk_ms * (args.dense / args.dense_sub) ** 2, 1)}
    assert c["clusters"] == 1
    res["cases"].append(c)
    print(json.dumps(c), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
