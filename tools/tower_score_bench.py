#!/usr/bin/env python3
"""K11 tower scores at BASELINE C2 (32 x 64^3): one TowerDetectionMetrics.update (K8 on the prediction and on the ground
truth, sn_tower_centroids, sn_tower_match) between HIP events -- eager, captured into a hipGraph and replayed, and split
into its parts (K8 x 2 / centroids / match, each on buffers of its own) -- beside the host path that the same result took
before: K8 x 2 on the device, then per tile TowerProposals.towers(b) (a copy of the tile's label grid and a synchronise),
sna.filter_towers, sna.aggregate_centroids and a numpy matching loop.
Ground truth: gt_occ of the golden TS40K sample (tests/golden/ts40k_sample575_full.npz) x 32; prediction: the same grid
OR-ed with itself shifted by one along axis 1, plus a block.  The bench checks what it times: the device's totals equal the
host path's.  Writes one JSON file.
    python tools/tower_score_bench.py --out profiles/tower_score_bench.json [--iters 50]"""
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
import scene_net_amd as sna  # noqa: E402
from scene_net_amd import _hip, tower_score  # noqa: E402

B, N = 32, 64
TAU, EPS, MIN_POINTS, MAX_TOWERS, HIT_DIST = 0.65, 3.5, 18, 64, 3.5


def timed(fn, iters, spin_ms=100.0):
    """ms per call by events over `iters` calls, after ~100 ms of the same work and a synchronise."""
    gc.collect()
    t0 = time.perf_counter()
    while (time.perf_counter() - t0) * 1e3 < spin_ms:
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def golden_grids(dev):
    a = np.load(os.path.join(ROOT, "tests", "golden", "ts40k_sample575_full.npz"))["tile"]
    batch = sna.PointBatch.from_tiles([a[:, :3]], [a[:, 3]], device=dev)
    g = sna.voxelize_batch(batch, (N, N, N), [15.0], want_occ=True, want_gt_occ=True, occ_dtype=torch.bool)
    gt = g.gt_occ[:, 0].expand(B, N, N, N).contiguous().cpu().numpy() != 0
    pred = gt.copy()
    pred[:, :, 1:, :] |= gt[:, :, :-1, :]
    pred[:, 40:60, 5:9, 50:54] = True
    return pred, gt


def host_update(pred_dev, gt_dev, metric):
    """the parent commit's way to the same totals: K8 x 2 on the device, the rest per tile on the host"""
    props = sna.tower_proposals(pred_dev, TAU, eps=EPS, min_points=MIN_POINTS, max_towers=MAX_TOWERS)
    gt_props = sna.tower_proposals(gt_dev, eps=EPS, min_points=MIN_POINTS, max_towers=MAX_TOWERS)
    center = props.grid_center()
    t = dict.fromkeys(tower_score.TOTAL_NAMES, 0)
    dist_total = 0.0
    for b in range(pred_dev.shape[0]):
        towers, cents = props.towers(b)
        if len(towers):
            towers, cents = sna.filter_towers(towers, cents, metric.threshold, center, tower_height=metric.tower_height,
                                              radius=metric.radius)
        agg = sna.aggregate_centroids(cents, min_euc=metric.min_euc)
        _, gt_c = gt_props.towers(b)
        gt_c = np.asarray(gt_c, dtype=np.float64).reshape(-1, 3)[:, 1:]
        hits, used = 0, set()
        for g in gt_c:
            if len(agg) == 0:
                continue
            d = np.linalg.norm(np.full_like(agg, g) - agg, axis=1)
            m = int(np.argmin(d))
            if d[m] <= metric.hit_dist:
                hits += 1
                used.add(m)
                dist_total += float(d[m])
        t["tiles"] += 1
        t["gt_towers"] += len(gt_c)
        t["proposals"] += len(agg)
        t["hits"] += hits
        t["misses"] += len(gt_c) - hits
        t["false_proposals"] += len(agg) - len(used)
    return [t[n] for n in tower_score.TOTAL_NAMES], dist_total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="tower_score_bench.json")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--host-iters", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tower_score_bench needs a HIP device (there is no CPU path)")
    dev = torch.device("cuda:0")
    pred_np, gt_np = golden_grids(dev)
    pred = torch.from_numpy(pred_np.astype(np.float32) * 0.9).to(dev)
    gt = torch.from_numpy(gt_np).to(dev)
    metric = sna.TowerDetectionMetrics(tau=TAU, eps=EPS, min_points=MIN_POINTS, hit_dist=HIT_DIST,
                                       max_towers=MAX_TOWERS).to(dev)

    # what is timed is right: the device's totals equal the host path's
    metric.update(pred, gt)
    want_totals, want_dist = host_update(pred, gt, metric)
    values = metric.compute()
    assert metric.totals.tolist() == want_totals, (metric.totals.tolist(), want_totals)
    assert abs(values["dist_total"] - want_dist) <= max(1, want_totals[4]) * 2.0 ** -53 * want_dist
    metric.reset()

    eager = timed(lambda: metric.update(pred, gt), args.iters)
    # the parts, each on outputs of its own
    k8_pred = timed(lambda: sna.tower_proposals(pred, TAU, eps=EPS, min_points=MIN_POINTS, max_towers=MAX_TOWERS), args.iters)
    k8_gt = timed(lambda: sna.tower_proposals(gt, eps=EPS, min_points=MIN_POINTS, max_towers=MAX_TOWERS), args.iters)
    props = sna.tower_proposals(pred, TAU, eps=EPS, min_points=MIN_POINTS, max_towers=MAX_TOWERS)
    gt_props = sna.tower_proposals(gt, eps=EPS, min_points=MIN_POINTS, max_towers=MAX_TOWERS)
    cents = sna.tower_centroids(props, metric.threshold)
    centroids = timed(lambda: sna.tower_centroids(props, metric.threshold), args.iters)
    totals = torch.zeros(_hip.SN_TSCORE_NTOTAL, dtype=torch.int64, device=dev)
    dist_total = torch.zeros(1, dtype=torch.float64, device=dev)
    match = timed(lambda: tower_score._match(cents, gt_props, 0, None, HIT_DIST, totals, dist_total), args.iters)
    match_plain = timed(lambda: tower_score._match(cents, gt_props, 0, None, HIT_DIST), args.iters)
    # captured
    metric.reset()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        metric.update(pred, gt)
    replay = timed(graph.replay, args.iters)
    del graph
    # the host path, a host clock around work that ends synchronised
    host_update(pred, gt, metric)
    host = []
    for _ in range(args.host_iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host_update(pred, gt, metric)
        host.append((time.perf_counter() - t0) * 1e3)
    host_ms = sorted(host)[len(host) // 2]

    res = {"device": torch.cuda.get_device_name(dev), "shape": [B, N, N, N], "tau": TAU, "eps": EPS,
           "min_points": MIN_POINTS, "max_towers": MAX_TOWERS, "hit_dist": HIT_DIST, "iters": args.iters,
           "totals": dict(zip(tower_score.TOTAL_NAMES, want_totals)), "values": {k: values[k] for k in
                                                                                ("recall", "precision", "f1", "mean_error")},
           "update_eager_us": round(eager * 1e3, 2), "update_graph_replay_us": round(replay * 1e3, 2),
           "parts_us": {"k8_pred": round(k8_pred * 1e3, 2), "k8_gt": round(k8_gt * 1e3, 2),
                        "centroids": round(centroids * 1e3, 2), "match_with_totals": round(match * 1e3, 2),
                        "match_without_totals": round(match_plain * 1e3, 2)},
           "host_path_ms": round(host_ms, 2), "host_path_runs_ms": [round(v, 2) for v in host],
           "host_path_over_eager": round(host_ms / eager, 1), "host_path_over_replay": round(host_ms / replay, 1),
           "note": "parts include the Python layer's output allocations; the host path is K8 x 2 on the device plus, per "
                   "tile, towers(b) for both sides, filter_towers, aggregate_centroids and the numpy matching loop"}
    print(json.dumps(res, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
