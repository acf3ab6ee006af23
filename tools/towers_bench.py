#!/usr/bin/env python3
"""K8 tower proposals at BASELINE C2 (32 x 64^3): sn_tower_proposals (sna.tower_proposals, six launches) between HIP
events -- the whole entry, each launch as the difference of two prefixes 1..k of the call (sn_tower_proposals_launches), and
the same call captured into a hipGraph and replayed -- on
  - gt_occ of the golden TS40K sample (tests/golden/ts40k_sample575_full.npz), replicated over the batch, and
  - synthetic grids at 0.5 %, 2 % and 10 % positives (half of them in solid blobs, half scattered),
beside the pipeline step of the same run (pipe(batch) on a batch resident in HBM, as tools/stream_bench.py case (e)) and
a host baseline on the same grids: the device-to-host copy plus the numpy oracle of the tests, and
sklearn.cluster.DBSCAN where it imports (both on a few tiles, scaled to the batch).  The bench checks what it times:
one tile of every set against the oracle.  Writes one JSON file.
    python tools/towers_bench.py --out profiles/towers_bench.json [--iters 50]"""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
import scene_net_amd as sna  # noqa: E402
from scene_net_amd import _hip  # noqa: E402
from scene_net_amd.synthetic import synthetic_tile  # noqa: E402
import towers_cases as tc  # noqa: E402

B, N = 32, 64
EPS, MIN_POINTS, MAX_TOWERS = 3.5, 18, 64
LAUNCHES = ("threshold", "core", "union", "flatten", "rank", "finish")


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


def synthetic_grids(fraction, seed):
    """bool [B, N, N, N]: `fraction` positives, half in solid 5 x 5 x 12 columns (tower-like), half scattered"""
    rng = np.random.default_rng(seed)
    g = rng.random((B, N, N, N)) < fraction / 2
    per_blob = 5 * 5 * 12
    blobs = max(1, int(fraction / 2 * N ** 3 / per_blob))
    for b in range(B):
        for _ in range(blobs):
            z, x, y = rng.integers(0, N - 12), rng.integers(0, N - 5), rng.integers(0, N - 5)
            g[b, z:z + 12, x:x + 5, y:y + 5] = True
    return g


def golden_grids(dev):
    a = np.load(os.path.join(ROOT, "tests", "golden", "ts40k_sample575_full.npz"))["tile"]
    batch = sna.PointBatch.from_tiles([a[:, :3]], [a[:, 3]], device=dev)
    g = sna.voxelize_batch(batch, (N, N, N), [15.0], want_occ=True, want_gt_occ=True, occ_dtype=torch.bool)
    return g.gt_occ[:, 0].expand(B, N, N, N).contiguous().cpu().numpy() != 0


def host_baseline(grid_dev, positive, tiles):
    """seconds for the batch on the host: the device-to-host copy of the whole batch (median of six .cpu() calls into
    pageable memory after one warm-up) and the clustering of `tiles` tiles, scaled to B"""
    copies = []
    for _ in range(7):                                    # pageable destination, as a plain .cpu() gives; the first is warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        grid_dev.cpu()
        copies.append(time.perf_counter() - t0)
    d2h = sorted(copies[1:])[len(copies[1:]) // 2]
    t0 = time.perf_counter()
    for b in range(tiles):
        tc.dbscan_grid(positive[b], EPS, MIN_POINTS, None, MAX_TOWERS)
    oracle = (time.perf_counter() - t0) * B / tiles
    out = {"d2h_ms": round(d2h * 1e3, 3), "oracle_ms_batch": round(oracle * 1e3, 2), "tiles_timed": tiles}
    try:
        from sklearn.cluster import DBSCAN
    except ImportError:
        out["sklearn_ms_batch"] = None
        return out
    t0 = time.perf_counter()
    for b in range(tiles):
        pts = np.argwhere(positive[b]).astype(np.float64)
        if len(pts):
            DBSCAN(eps=EPS, min_samples=MIN_POINTS).fit(pts)
    out["sklearn_ms_batch"] = round((time.perf_counter() - t0) * B / tiles * 1e3, 2)
    return out


def grid_case(name, positive, dev, iters, pipe_ms, host_tiles):
    grid = torch.from_numpy(positive).to(dev)             # bool, as gt_occ and prob_to_label's output arrive
    ws = torch.empty(_hip.towers_ws_bytes(B, N, N, N) // 8, dtype=torch.int64, device=dev)
    labels = torch.empty((B, N, N, N), dtype=torch.int32, device=dev)
    n_towers = torch.empty(B, dtype=torch.int32, device=dev)
    stats = torch.empty((B, MAX_TOWERS, _hip.SN_TOWER_NSTAT), dtype=torch.int64, device=dev)

    def entry(launches=None):
        _hip.tower_proposals(grid, 0.5, EPS, MIN_POINTS, MAX_TOWERS, ws, labels, n_towers, stats, launches=launches)
    entry()
    torch.cuda.synchronize()
    want = tc.dbscan_grid(positive[0], EPS, MIN_POINTS, None, MAX_TOWERS)
    assert np.array_equal(labels[0].cpu().numpy(), want[0]) and int(n_towers[0]) == want[1]
    assert np.array_equal(stats[0].cpu().numpy(), want[2])
    whole = timed(entry, iters)
    # per launch: the prefixes 1..k, each from a fresh start (launch 2 resets parent[v] = v, so the union and the flatten
    # do their real work every time), and the differences between neighbouring prefixes
    prefix = [0.0] + [timed(lambda k=k: entry((1, k)), iters) for k in range(1, len(LAUNCHES) + 1)]
    per = {name: round((prefix[k] - prefix[k - 1]) * 1e3, 2) for k, name in enumerate(LAUNCHES, start=1)}
    entry()
    alloc = timed(lambda: sna.tower_proposals(grid, eps=EPS, min_points=MIN_POINTS, max_towers=MAX_TOWERS), iters)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        entry()
    replay = timed(graph.replay, iters)
    host = host_baseline(grid, positive, host_tiles)
    host_ms = host["d2h_ms"] + host["oracle_ms_batch"]
    res = {"case": name, "positives_fraction": round(float(positive.mean()), 5),
           "towers_per_tile_mean": round(float(n_towers.float().mean()), 2),
           "entry_us": round(whole * 1e3, 2), "entry_with_allocation_us": round(alloc * 1e3, 2),
           "graph_replay_us": round(replay * 1e3, 2), "launch_us": per, "launch_sum_us": round(sum(per.values()), 2),
           "prefix_us": [round(v * 1e3, 2) for v in prefix[1:]],
           "dominant_launch": max(per, key=per.get), "pipeline_step_us": round(pipe_ms * 1e3, 2),
           "entry_over_pipeline_step": round(whole / pipe_ms, 3), "host": host,
           "host_oracle_over_entry": round(host_ms / whole, 1),
           "host_sklearn_over_entry": (round((host["d2h_ms"] + host["sklearn_ms_batch"]) / whole, 1)
                                       if host["sklearn_ms_batch"] is not None else None)}
    del graph
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="towers_bench.json")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--host-tiles", type=int, default=2, help="tiles the host baseline clusters (scaled to the batch)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("towers_bench needs a HIP device (there is no CPU path)")
    dev = torch.device("cuda:0")
    # the pipeline step of the same run: pipe(batch) on a resident batch
    torch.manual_seed(0)
    model = sna.SceneNet({"cy": 2, "cone": 1, "neg": 1}, (9, 9, 9)).to(dev)
    pipe = sna.ScenePipeline(model, (N, N, N), keep_labels=[15.0])
    tiles, labs = zip(*[synthetic_tile(i, 100_000) for i in range(B)])
    batch = sna.PointBatch.from_tiles(tiles, labs, device=dev)

    def step():
        with torch.no_grad():
            return pipe(batch)
    pipe_ms = timed(step, args.iters)
    res = {"device": torch.cuda.get_device_name(dev), "shape": [B, N, N, N], "eps": EPS, "min_points": MIN_POINTS,
           "max_towers": MAX_TOWERS, "pipeline_step_us": round(pipe_ms * 1e3, 2), "cases": []}
    sets = [("golden gt_occ x 32", golden_grids(dev))]
    sets += [(f"synthetic {100 * f:g} %", synthetic_grids(f, seed)) for seed, f in enumerate((0.005, 0.02, 0.10))]
    for name, positive in sets:
        c = grid_case(name, positive, dev, args.iters, pipe_ms, args.host_tiles)
        res["cases"].append(c)
        print(f"{name:22s} entry {c['entry_us']:9.2f} us  replay {c['graph_replay_us']:9.2f} us  "
              f"({c['entry_over_pipeline_step']:.2f} x the pipeline step of {c['pipeline_step_us']} us)  "
              f"dominant: {c['dominant_launch']} {c['launch_us'][c['dominant_launch']]} us  "
              f"host oracle {c['host']['oracle_ms_batch']} ms, sklearn {c['host']['sklearn_ms_batch']} ms", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
