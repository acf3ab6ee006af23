#!/usr/bin/env python3
"""Feeding the pipeline from disk: the parent loader (TS40KTiles.load_batch) against TileStream, in one process, on the
same batch shape (C2: 32 tiles x 100k points, synthetic tiles written to a temporary directory; the page cache is WARM:
the files were written moments before they are read, so (d) measures the host path, not a disk).

  (a) h2d_GBps      pinned host-to-device rate of one batch-sized buffer, warm, median
  (b) parent        tiles/s of ScenePipeline fed by the ds.load_batch loop
  (c) stream_ram    tiles/s fed by TileStream, the readers' file read replaced by a memcpy from preloaded arrays
  (d) stream_files  tiles/s fed by TileStream from the .npy files
  (e) resident      tiles/s of the same pipeline on a batch resident in HBM
  (f) unpack        sn_tiles_unpack alone between events, over buffer sets that together exceed the last-level cache,
                    and its share of (c)'s time per batch
(b) and (d) alternate in the same run; every rate is reported with the spread over the rounds.
Writes profiles/stream_bench.json.  Needs a GPU: python tools/stream_bench.py [--rounds 5]"""
import argparse
import gc
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import scene_net_amd as sna  # noqa: E402
from scene_net_amd import _hip, stream as st  # noqa: E402
from scene_net_amd.synthetic import apply_bank_spec, synthetic_bank_spec, synthetic_tile  # noqa: E402

GENEO_NUM, KERNEL_SIZE = {"cy": 6, "cone": 5, "neg": 5}, (9, 9, 9)


def spread(values):
    return {"median": statistics.median(values), "min": min(values), "max": max(values), "n": len(values),
            "spread": max(values) - min(values)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--points", type=int, default=100_000)
    ap.add_argument("--files", type=int, default=128)
    ap.add_argument("--grid", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--stream-epochs", type=int, default=3, help="epochs per timed round of a streamed path")
    ap.add_argument("--readers", type=int, default=4)
    ap.add_argument("--slots", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("stream_bench needs a HIP device: nothing here can be measured without one")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    B, n_batches = args.batch, args.files // args.batch
    assert n_batches >= 2, "--files must hold at least two batches"

    specs, names, lambdas, last = synthetic_bank_spec(GENEO_NUM)
    torch.manual_seed(0)
    model = sna.SceneNet(GENEO_NUM, KERNEL_SIZE)
    apply_bank_spec(model, specs, names, lambdas, last)
    model = model.to(dev)
    pipe = sna.ScenePipeline(model, (args.grid,) * 3)

    def compute(batch):
        with torch.no_grad():
            return pipe(batch)

    with tempfile.TemporaryDirectory(prefix="stream_bench_") as root:
        os.mkdir(os.path.join(root, "fit"))
        distinct = [np.concatenate([x, l[:, None]], axis=1) for x, l in
                    (synthetic_tile(20_000 + t, args.points) for t in range(min(args.files, B)))]
        for k in range(args.files):
            np.save(os.path.join(root, "fit", f"sample_{k:04d}.npy"), distinct[k % len(distinct)])
        ds = sna.TS40KTiles(root, "fit")
        infos = sna.scan_tiles(ds)
        assert all(i.ok for i in infos)
        tile_bytes = args.points * 32
        batch_bytes = B * tile_bytes
        batches = [list(range(k * B, (k + 1) * B)) for k in range(n_batches)]
        preloaded = {os.path.join(ds.dataset_path, str(f)): distinct[k % len(distinct)] for k, f in enumerate(ds.npy_files)}

        # (e) resident, and the warm-up of every kernel the timed loops use
        resident = ds.load_batch(batches[0], device=dev)
        for _ in range(5):
            compute(resident)
        torch.cuda.synchronize()
        gc.collect()
        gc.freeze()

        def time_resident(steps=100):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                compute(resident)
            torch.cuda.synchronize()
            return steps * B / (time.perf_counter() - t0)

        def time_parent():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for idx in batches:
                compute(ds.load_batch(idx, device=dev))
            torch.cuda.synchronize()
            return len(batches) * B / (time.perf_counter() - t0)

        stream = sna.TileStream(ds, B, device=dev, slots=args.slots, readers=args.readers, timeout_s=60)

        def time_stream():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            n = 0
            for _ in range(args.stream_epochs):
                for batch in stream:
                    compute(batch)
                    n += len(batch.sizes)
            torch.cuda.synchronize()
            return n / (time.perf_counter() - t0)

        # (a) pinned host-to-device rate of one batch-sized buffer
        host = torch.empty(batch_bytes // 8, dtype=torch.float64).pin_memory()
        host.normal_()
        d_rows = torch.empty(batch_bytes // 8, dtype=torch.float64, device=dev)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        h2d = []
        for k in range(9):
            ev[0].record()
            d_rows.copy_(host, non_blocking=True)
            ev[1].record()
            torch.cuda.synchronize()
            if k >= 2:
                h2d.append(batch_bytes / (ev[0].elapsed_time(ev[1]) * 1e-3) / 1e9)

        # (f) the unpack kernel alone.  One batch of rows and its outputs are 2 x 102.4 MB, less than the 256 MiB last-level
        # cache, so a loop over ONE set could be served from it: the HBM figure rotates over `sets` sets (together well
        # past the cache; a set comes round again after all the others went through); the same-set figure is kept beside it
        total = batch_bytes // 32
        sets = max(4, -(-3 * 256 * 2**20 // (2 * batch_bytes)) + 1)
        bufs = [(torch.randn((total, 4), dtype=torch.float64, device=dev),
                 torch.empty((total, 3), dtype=torch.float64, device=dev),
                 torch.empty((total,), dtype=torch.float64, device=dev)) for _ in range(sets)]
        off = torch.arange(0, total + 1, args.points, dtype=torch.int64, device=dev)
        bad = torch.zeros((B,), dtype=torch.int32, device=dev)

        def time_unpack(pick, reps=12, warm=sets):
            out = []
            for k in range(warm + reps):
                rows, pts, lab = bufs[pick(k)]
                ev[0].record()
                _hip.tiles_unpack(rows, pts, lab, off, bad)
                ev[1].record()
                torch.cuda.synchronize()
                if k >= warm:
                    out.append(ev[0].elapsed_time(ev[1]))
            return out
        unpack_ms = time_unpack(lambda k: k % sets)
        unpack_same_ms = time_unpack(lambda k: 0)
        del host, d_rows, bufs

        # warm both loaders once, then alternate (b) and (d)
        time_parent()
        time_stream()
        parent, files, res = [], [], []
        for _ in range(args.rounds):
            parent.append(time_parent())
            files.append(time_stream())
            res.append(time_resident())
        # (c): the same stream, the file read replaced by a memcpy
        real_read = st._read_tile

        def from_ram(path, info, out):
            out[...] = preloaded[path]
        st._read_tile = from_ram
        try:
            time_stream()
            ram = [time_stream() for _ in range(args.rounds)]
        finally:
            st._read_tile = real_read
            stream.close()

    a, b, c, d, e = spread(h2d), spread(parent), spread(ram), spread(files), spread(res)
    up = statistics.median(unpack_ms)
    c_ms_per_batch = B / c["median"] * 1e3
    h2d_ms = batch_bytes / (a["median"] * 1e9) * 1e3
    comp_ms = B / e["median"] * 1e3
    result = {
        "shape": {"batch": B, "points_per_tile": args.points, "files": args.files, "grid": args.grid,
                  "tile_bytes_raw_rows": tile_bytes, "readers": args.readers, "slots": args.slots,
                  "stream_epochs_per_round": args.stream_epochs, "rounds": args.rounds},
        "page_cache": "warm (files written by this process just before they are read)",
        "device": torch.cuda.get_device_name(dev),
        "a_h2d_GBps": a,
        "b_parent_tiles_per_s": b,
        "c_stream_ram_tiles_per_s": c,
        "d_stream_files_tiles_per_s": d,
        "e_resident_tiles_per_s": e,
        "f_unpack": {"what": f"rotating over {sets} sets of rows + outputs ({sets * 2 * batch_bytes / 2**20:.0f} MiB in all): "
                             "every call reads rows that left the last-level cache",
                     "ms": up, "ms_min": min(unpack_ms), "ms_max": max(unpack_ms),
                     "GBps_read_plus_written": 2 * batch_bytes / (up * 1e-3) / 1e9,
                     "share_of_c_batch_time": up / c_ms_per_batch,
                     "same_set_ms": statistics.median(unpack_same_ms),
                     "same_set_GBps_read_plus_written": 2 * batch_bytes / (statistics.median(unpack_same_ms) * 1e-3) / 1e9,
                     "same_set_note": "one set reused: 195 MiB, may be served from the 256 MiB last-level cache"},
        "frac_of_measured_h2d": c["median"] * tile_bytes / (a["median"] * 1e9),
        # of one batch's compute time, the part that does not show in (c)'s time per batch next to the batch's own
        # transfer and unpack: (h2d + unpack + compute - c) / compute, clipped to 0..1
        "compute_hidden_fraction": max(0.0, min(1.0, (h2d_ms + up + comp_ms - c_ms_per_batch) / comp_ms)),
        "ms_per_batch": {"c": c_ms_per_batch, "h2d_at_a": h2d_ms, "compute_at_e": comp_ms, "unpack": up},
        "d_over_b": d["median"] / b["median"],
        "d_beats_b_by_more_than_both_spreads": (d["median"] - b["median"]) > (d["spread"] + b["spread"]),
    }
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
