#!/usr/bin/env python3
"""K14 SemanticKITTI decode on a batch of 32 synthetic scans of 1.2 * 10^5 points (the size of BASELINE's C4 scans).
Everything is measured in this one run, after a warm-up, per call between HIP events (kernels) or by the host clock around
work that ends in a synchronise (file reads); reported as the median with the minimum and the maximum:
  (a) sn_kitti_decode alone (pts, labels and the per-scan census of 260 classes; then with remission and instance as
      well), rotating over buffer sets so that no call finds its rows in the 256 MiB last-level cache;
  (b) sn_tiles_unpack (K7) on the same f32 rows (cols 4, labels wanted) and the same rotated buffers, in the same run.
      The yardstick is that time x 52 / 48, the ratio of the bytes the two move per point (x 60 / 48 with remission and
      instance); the decode is meant to stay within 25 % of it (the second input stream and the census are work K7 does
      not have).  A reported figure, not an assertion.
  (c) KittiReader.read of the 32 file pairs, page cache warm: total time, and file bytes per second against the rate of a
      pinned host-to-device copy of the same size measured here.
  (d) the host path: np.fromfile, reshape, `& 0xFFFF`, astype(float64) and an upload per scan -- what a user writes today.
The bench checks what it times against (d)'s arrays, bit for bit.  One JSON file.
    python tools/kitti_bench.py --out profiles/kitti_bench.json [--scans 32] [--points 120000] [--iters 40]"""
import argparse
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
from scene_net_amd import _hip  # noqa: E402
from scene_net_amd.kitti import KittiReader  # noqa: E402

HBM_PEAK = 8.0e12      # bytes / s, the part's specification
MARGIN = 1.25
N_HIST = 260
# SemanticKITTI's raw classes with a road-scene mix: a few classes carry nearly all points, which is what the LDS census has
# to live with
CLASSES = np.array([40, 70, 50, 48, 72, 10, 51, 44, 71, 80, 0, 30, 81, 252], dtype=np.uint32)
CLASS_P = [.25, .27, .15, .12, .08, .04, .03, .02, .015, .005, .01, .003, .002, .005]


def spread(samples):
    return {"median": round(statistics.median(samples), 2), "min": round(min(samples), 2), "max": round(max(samples), 2),
            "n": len(samples)}


def per_call_us(calls, iters, warm=3):
    """us per call by one event pair per call; calls[i % len(calls)] is call i (each works on its own buffer set)"""
    for i in range(warm * len(calls)):
        calls[i % len(calls)]()
    torch.cuda.synchronize()
    pairs = []
    for i in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        calls[i % len(calls)]()
        b.record()
        pairs.append((a, b))
    torch.cuda.synchronize()
    return [a.elapsed_time(b) * 1e3 for a, b in pairs]


def synthetic_scan(n, seed):
    rng = np.random.default_rng(seed)
    rows = (rng.standard_normal((n, 4)) * [30.0, 30.0, 2.0, 0.3]).astype("<f4")
    sem = rng.choice(CLASSES, size=n, p=CLASS_P)
    words = (sem | (rng.integers(0, 200, n, dtype=np.uint32) << 16)).astype("<u4")
    return rows, words


def host_decode(bin_path, label_path):
    """what a user writes today: (xyz [n,3] f64, gt [n] f64)"""
    scan = np.fromfile(bin_path, dtype=np.float32).reshape((-1, 4))
    label = np.fromfile(label_path, dtype=np.uint32)
    return scan[:, :3].astype(np.float64), (label & 0xFFFF).astype(np.float64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="kitti_bench.json")
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--scans", type=int, default=32)
    ap.add_argument("--points", type=int, default=120_000)
    ap.add_argument("--sets", type=int, default=4, help="buffer sets the kernels rotate over")
    ap.add_argument("--tmp", default=None, help="directory for the synthetic files (default: a temporary one)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("kitti_bench needs a HIP device (there is no CPU path)")
    dev = torch.device("cuda:0")
    B, n = args.scans, args.points
    sizes = [n - 37 * (b % 5) for b in range(B)]          # scans differ a little in size, as real ones do
    total = sum(sizes)
    scans = [synthetic_scan(sizes[b], b) for b in range(B)]
    rows_np = np.concatenate([s[0] for s in scans])
    words_np = np.concatenate([s[1] for s in scans])
    offsets = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int64, device=dev)

    with tempfile.TemporaryDirectory(dir=args.tmp) as tmp:
        bins, labels = [], []
        for b, (rows, words) in enumerate(scans):
            bins.append(os.path.join(tmp, f"{b:06d}.bin"))
            labels.append(os.path.join(tmp, f"{b:06d}.label"))
            rows.tofile(bins[-1])
            words.tofile(labels[-1])

        # (d) the host path (also the reference values of this batch)
        host_ms = []
        for _ in range(3):
            t0 = time.perf_counter()
            outs = []
            for b in range(B):
                xyz, gt = host_decode(bins[b], labels[b])
                outs.append((torch.from_numpy(xyz).to(dev), torch.from_numpy(gt).to(dev)))
            torch.cuda.synchronize()
            host_ms.append((time.perf_counter() - t0) * 1e3)
        want_pts = torch.cat([o[0] for o in outs])
        want_lab = torch.cat([o[1] for o in outs])
        want_hist = torch.stack([torch.bincount(o[1].to(torch.int64), minlength=N_HIST)[:N_HIST] for o in outs])
        del outs

        # (a), (b) the kernels alone on rotated buffer sets
        sets = []
        for _ in range(args.sets):
            sets.append({"rows": torch.from_numpy(rows_np).to(dev), "words": torch.from_numpy(words_np.view(np.int32)).to(dev),
                         "pts": torch.empty((total, 3), dtype=torch.float64, device=dev),
                         "labels": torch.empty((total,), dtype=torch.float64, device=dev),
                         "rem": torch.empty((total,), dtype=torch.float32, device=dev),
                         "inst": torch.empty((total,), dtype=torch.int32, device=dev),
                         "hist": torch.zeros((B, N_HIST), dtype=torch.int64, device=dev),
                         "bad": torch.zeros((B,), dtype=torch.int32, device=dev)})
        assert all(s["rows"].data_ptr() % 16 == 0 for s in sets)

        def decode(s, full, bad):
            _hip.kitti_decode(s["rows"], s["words"], total, offsets, s["pts"], s["labels"], None,
                              s["rem"] if full else None, s["inst"] if full else None, s["hist"], s["bad"] if bad else None)

        decode(sets[0], True, True)
        torch.cuda.synchronize()
        assert torch.equal(sets[0]["pts"].view(torch.int64), want_pts.view(torch.int64)), "decode differs from the host path"
        assert torch.equal(sets[0]["labels"], want_lab) and torch.equal(sets[0]["hist"], want_hist)
        assert int(sets[0]["bad"].sum()) == 0
        assert torch.equal(sets[0]["rem"].view(torch.int32), sets[0]["rows"][:, 3].contiguous().view(torch.int32))

        unpack_us = per_call_us([lambda s=s: _hip.tiles_unpack(s["rows"], s["pts"], s["labels"]) for s in sets], args.iters)
        base_us = per_call_us([lambda s=s: decode(s, False, False) for s in sets], args.iters)
        unpack2_us = per_call_us([lambda s=s: _hip.tiles_unpack(s["rows"], s["pts"], s["labels"]) for s in sets], args.iters)
        bad_us = per_call_us([lambda s=s: decode(s, False, True) for s in sets], args.iters)
        full_us = per_call_us([lambda s=s: decode(s, True, False) for s in sets], args.iters)
        del sets
        unpack_all = unpack_us + unpack2_us              # (the yardstick was taken before and after the decode)
        yard = statistics.median(unpack_all)

        # (c) the reader, page cache warm, and a pinned copy of the same size
        file_bytes = 20 * total
        reader = KittiReader(dev, batch_bytes=max(64 << 20, file_bytes))
        got = reader.read(bins, labels, n_hist=N_HIST)
        torch.cuda.synchronize()
        assert torch.equal(got.pts.view(torch.int64), want_pts.view(torch.int64)) and torch.equal(got.labels, want_lab)
        assert torch.equal(got.hist, want_hist)
        read_ms = []
        for _ in range(7):
            del got
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got = reader.read(bins, labels, n_hist=N_HIST)
            torch.cuda.synchronize()
            read_ms.append((time.perf_counter() - t0) * 1e3)
        del got
        host, raw = torch.empty(file_bytes, dtype=torch.uint8).pin_memory(), torch.empty(file_bytes, dtype=torch.uint8, device=dev)
        h2d_us = per_call_us([lambda: raw.copy_(host, non_blocking=True)], 10)
        h2d_rate = file_bytes / (statistics.median(h2d_us) * 1e-6)

    def case(us, bytes_per_point):
        med = statistics.median(us)
        y = yard * bytes_per_point / 48
        return {"us": spread(us), "bytes_per_point": bytes_per_point,
                "bytes_per_s": round(total * bytes_per_point / (med * 1e-6), 0),
                "hbm_share": round(total * bytes_per_point / (med * 1e-6) / HBM_PEAK, 3), "yardstick_us": round(y, 2),
                "over_yardstick": round(med / y, 3), "margin": MARGIN, "within_margin": bool(med <= MARGIN * y)}

    read_med = statistics.median(read_ms)
    res = {"device": torch.cuda.get_device_name(dev), "scans": B, "points": total, "chunk_points": _hip.kitti_chunk_points(),
           "buffer_sets": args.sets, "hbm_peak_bytes_per_s": HBM_PEAK, "n_hist": N_HIST,
           "tiles_unpack_us": spread(unpack_all), "tiles_unpack_before_us": spread(unpack_us),
           "tiles_unpack_after_us": spread(unpack2_us),
           "tiles_unpack_hbm_share": round(total * 48 / (yard * 1e-6) / HBM_PEAK, 3),
           "yardstick": "sn_tiles_unpack (f32 rows of 4 columns, labels wanted, the same rows) in the same run, times "
                        "bytes_per_point / 48; margin 1.25",
           "decode": case(base_us, 52), "decode_with_bad": case(bad_us, 52), "decode_remission_instance": case(full_us, 60),
           "reader_ms": spread(read_ms), "reader_file_bytes": file_bytes,
           "reader_file_bytes_per_s": round(file_bytes / (read_med * 1e-3), 0),
           "pinned_h2d_us": spread(h2d_us), "pinned_h2d_bytes_per_s": round(h2d_rate, 0),
           "reader_share_of_pinned_h2d": round(file_bytes / (read_med * 1e-3) / h2d_rate, 3),
           "host_path_ms": spread(host_ms), "host_over_reader": round(statistics.median(host_ms) / read_med, 2),
           "host_path": "np.fromfile, reshape, & 0xFFFF, astype(float64), one upload per array and scan"}
    for name in ("decode", "decode_with_bad", "decode_remission_instance"):
        c = res[name]
        print(f"{name:26s} {c['us']['median']:8.1f} us [{c['us']['min']:.1f}, {c['us']['max']:.1f}] = {c['hbm_share']:.2f} of "
              f"HBM peak, / yardstick {c['over_yardstick']:.2f}", flush=True)
    print(f"sn_tiles_unpack {yard:.1f} us = {res['tiles_unpack_hbm_share']:.2f} of HBM peak; reader {read_med:.1f} ms = "
          f"{res['reader_file_bytes_per_s'] / 1e9:.2f} GB/s of {h2d_rate / 1e9:.1f} GB/s pinned; host path "
          f"{statistics.median(host_ms):.1f} ms", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
