#!/usr/bin/env python3
"""The kernels of K12 and of K9's count pass under rocprofv3, on the scan and the three region sets of tools/census_bench.py
(32 and 128 discs at towers, the 32-box lattice).  Two roles:

  the profiled program (12 sn_crop_census calls, then 12 sn_crop_count calls per region set, in that order):
      rocprofv3 --kernel-trace --stats --output-format csv -d OUT/trace -- python3 tools/census_profile.py
      rocprofv3 --pmc SQ_INSTS_VALU SQ_INSTS_SALU SQ_WAVE_CYCLES SQ_WAIT_ANY --output-format csv -d OUT/pmc1 -- python3 tools/census_profile.py
      rocprofv3 --pmc TCC_EA0_ATOMIC_sum --output-format csv -d OUT/pmc2 -- python3 tools/census_profile.py
      rocprofv3 --pmc FETCH_SIZE --output-format csv -d OUT/pmc3 -- python3 tools/census_profile.py
  (counters in runs of their own, never together with a trace)

  the summary, which needs no GPU: per kernel and region set the mean over the last 10 of its 12 dispatches, written under
  "profile" into the bench's JSON:
      python3 tools/census_profile.py --summarise OUT/trace OUT/pmc1 OUT/pmc2 OUT/pmc3 --into profiles/census_bench.json
"""
import argparse
import collections
import csv
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

LAUNCHES, SKIP = 12, 2
CASES = ("discs K=32", "discs K=128", "box lattice K=32")
KERNELS = {"crop_census_kernel": "census", "crop_census_decode_kernel": "census_decode", "crop_count_kernel": "count",
           "crop_prefix_kernel": "count_prefix", "crop_offsets_kernel": "count_offsets"}


def run(points):
    import numpy as np
    import torch
    from scene_net_amd import _hip
    from scene_net_amd.census import watch_trunc
    from scene_net_amd.crops import lattice_boxes
    from crops_bench import synthetic_scan
    dev = torch.device("cuda:0")
    xyz, lab, towers = synthetic_scan(points)
    pts, labels = torch.from_numpy(xyz).to(dev), torch.from_numpy(lab).to(dev)
    n = pts.shape[0]
    order = np.random.default_rng(0).permutation(len(towers))
    sets = [(np.column_stack([towers[order[:K], :2], np.full(K, 15.0), np.zeros(K)]), np.zeros(K, dtype=np.int32)) for K in (32, 128)]
    lo, hi = xyz[:, :2].min(axis=0), xyz[:, :2].max(axis=0)
    sets.append((lattice_boxes(lo, hi, 60.0, overlap=0.0), np.ones(32, dtype=np.int32)))
    watch = watch_trunc([15], device=dev)
    for rows, kinds_np in sets:
        K = rows.shape[0]
        regions, kinds = torch.from_numpy(rows).to(dev), torch.from_numpy(kinds_np).to(dev)
        ws = torch.empty(_hip.crop_census_ws_bytes(n, K, 1) // 8, dtype=torch.int64, device=dev)
        counts = torch.empty((K, 3), dtype=torch.int64, device=dev)
        rng = torch.empty((K, 2), dtype=torch.float64, device=dev)
        cws = torch.empty(_hip.crops_ws_bytes(n, K) // 8, dtype=torch.int64, device=dev)
        offsets = torch.empty(K + 1, dtype=torch.int64, device=dev)
        for _ in range(LAUNCHES):
            _hip.crop_census(pts, labels, regions, kinds, watch, ws, counts, rng)
        for _ in range(LAUNCHES):
            _hip.crop_count(pts, regions, kinds, cws, offsets)
        torch.cuda.synchronize()
    print("census_profile: done")


def short(name):
    for k in KERNELS:
        if k + "<" in name or name.endswith(k) or k + "(" in name:
            return KERNELS[k]
    return None


def per_case(values):
    """values of one kernel in dispatch order -> mean of the last LAUNCHES - SKIP per region set (None if the count is off)"""
    if len(values) != LAUNCHES * len(CASES):
        return None
    return [sum(values[c * LAUNCHES + SKIP:(c + 1) * LAUNCHES]) / (LAUNCHES - SKIP) for c in range(len(CASES))]


def summarise(dirs, into):
    out = {"_note": f"rocprofv3 over tools/census_profile.py ({LAUNCHES} dispatches per kernel and region set, mean of the last "
                    f"{LAUNCHES - SKIP}); kernel_us from a --kernel-trace --stats run, counters from --pmc runs of their own",
           "cases": list(CASES), "kernel_us": {}, "counters": {}}
    for d in dirs:
        for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
            rows = sorted(csv.DictReader(open(f)), key=lambda r: int(r["Start_Timestamp"]))
            acc = collections.defaultdict(list)
            for r in rows:
                k = short(r["Kernel_Name"])
                if k:
                    acc[k].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3)
            for k, v in acc.items():
                m = per_case(v)
                out["kernel_us"][k] = [round(x, 2) for x in m] if m else {"dispatches": len(v)}
        for f in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
            acc = collections.defaultdict(lambda: collections.defaultdict(float))
            for r in csv.DictReader(open(f)):
                k = short(r["Kernel_Name"])
                if k:
                    acc[(k, r["Counter_Name"])][int(r["Dispatch_Id"])] += float(r["Counter_Value"])
            for (k, c), by_id in acc.items():
                m = per_case([by_id[i] for i in sorted(by_id)])
                out["counters"].setdefault(k, {})[c] = [round(x, 1) for x in m] if m else {"dispatches": len(by_id)}
    res = json.load(open(into))
    res["profile"] = out
    json.dump(res, open(into, "w"), indent=1)
    print(json.dumps(out, indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--summarise", nargs="+", metavar="DIR")
    ap.add_argument("--into", default=os.path.join(ROOT, "profiles", "census_bench.json"))
    args = ap.parse_args()
    if args.summarise:
        summarise(args.summarise, args.into)
    else:
        run(args.points)


if __name__ == "__main__":
    main()
