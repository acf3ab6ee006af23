#!/usr/bin/env python3
"""K13 LAS decode on synthetic files of 10^7 points in the point formats 1 (28 B), 3 (34 B) and 6 (30 B), point data at an
odd offset.  Everything is measured in this one run, after a warm-up, per call between HIP events (kernels) or by the host
clock around work that ends in a synchronise (file reads); reported as the median with the minimum and the maximum:
  (a) sn_las_decode alone, rotating over buffer sets so that no call finds its bytes in the 256 MiB last-level cache;
      next to it sn_tiles_unpack (K7: f64 rows of 4 columns, the same n) on rotated buffers in the same run.  The yardstick
      is that time x (S + 32) / 64, the ratio of the bytes the two move per point; the decode is meant to stay within 25 %
      of it (the LDS staging is work K7 does not have).  A reported figure, not an assertion.
  (b) LasReader.read of the file, page cache warm: total time, and file bytes per second against the rate of a pinned
      host-to-device copy of one chunk measured here.
  (c) the host baseline: numpy's structured decode of the same file, `X * scale + offset` per column,
      np.vstack(...).transpose(), the class column, then the upload of both arrays.  It stands in for laspy's read and the
      reference's las_to_numpy; laspy itself is not installed where this runs.
The bench checks what it times against (c)'s arrays, bit for bit.  One JSON file.
    python tools/las_bench.py --out profiles/las_bench.json [--points 10000000] [--iters 20]"""
import argparse
import json
import os
import statistics
import struct
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from scene_net_amd import _hip  # noqa: E402
from scene_net_amd.las import LAS_STANDARD_LENGTH, LasReader, read_las_header  # noqa: E402

HBM_PEAK = 8.0e12      # bytes / s, the part's specification
MARGIN = 1.25
SCALE, OFFSET = (0.01, 0.01, 0.01), (5.0e5, 4.6e6, 100.0)
CLASS_BYTE = {1: 15, 3: 15, 6: 16}
# a TS40K-like class mix: a few classes carry nearly all points, which is what the LDS histogram has to live with
CLASSES, CLASS_P = np.array([2, 3, 4, 5, 1, 14, 15, 16], dtype=np.uint8), [.38, .2, .15, .2, .04, .015, .005, .01]


def spread(samples):
    return {"median": round(statistics.median(samples), 2), "min": round(min(samples), 2), "max": round(max(samples), 2),
            "n": len(samples)}


def per_call_us(calls, iters, warm=5):
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


def synthetic_records(n, fmt, seed=0):
    """[n, S] uint8: 2^20 random records repeated -- every byte random, the class byte drawn from the class mix"""
    S = LAS_STANDARD_LENGTH[fmt]
    rng = np.random.default_rng(seed + fmt)
    block = rng.integers(0, 256, size=(min(n, 1 << 20), S), dtype=np.uint8)
    flags = (rng.integers(0, 8, block.shape[0], dtype=np.uint8) << 5) if fmt <= 5 else 0   # formats 0..5: flag bits on top
    block[:, CLASS_BYTE[fmt]] = rng.choice(CLASSES, size=block.shape[0], p=CLASS_P) | flags
    return np.tile(block, (-(-n // block.shape[0]), 1))[:n]


def write_file(path, rows, fmt, pad):
    """a LAS 1.2 (formats 1, 3) or 1.4 (format 6) file; returns the data offset"""
    minor = 4 if fmt >= 6 else 2
    size = 375 if minor == 4 else 227
    n, S = rows.shape
    h = bytearray(size)
    h[0:4] = b"LASF"
    h[24], h[25] = 1, minor
    struct.pack_into("<HI", h, 94, size, size + pad)
    struct.pack_into("<BHI", h, 104, fmt, S, n if fmt <= 5 else 0)
    struct.pack_into("<3d", h, 131, *SCALE)
    struct.pack_into("<3d", h, 155, *OFFSET)
    if minor == 4:
        struct.pack_into("<Q", h, 247, n)
    with open(path, "wb") as f:
        f.write(h)
        f.write(bytes(pad))
        rows.tofile(f)
    return size + pad


def host_decode(path):
    """what laspy's read and las_to_numpy do, in numpy: (xyz [n,3] f64, classes [n] u8)"""
    h = read_las_header(path)
    fields = [("X", "<i4"), ("Y", "<i4"), ("Z", "<i4"), ("skip", "V3"), ("b15", "u1"), ("b16", "u1"),
              ("rest", f"V{h.record_length - 17}")]
    rec = np.fromfile(path, dtype=np.dtype(fields), count=h.n_points, offset=h.data_offset)
    x, y, z = (rec[c] * h.scale[a] + h.offset[a] for a, c in enumerate("XYZ"))
    pcnp = np.vstack((x, y, z)).transpose()
    classes = np.array((rec["b15"] & 31) if h.point_format <= 5 else rec["b16"])
    return pcnp, classes


def bench_format(fmt, n, iters, tmp, dev, reader, unpack_us):
    S = LAS_STANDARD_LENGTH[fmt]
    rows = synthetic_records(n, fmt)
    path = os.path.join(tmp, f"format{fmt}.las")
    off = write_file(path, rows, fmt, pad=6 if (375 if fmt >= 6 else 227) % 2 else 7)
    assert off % 2 == 1

    # (c) the host baseline (also the reference values of this file)
    host_ms, upload_ms = [], []
    for _ in range(3):
        t0 = time.perf_counter()
        pcnp, classes = host_decode(path)
        t1 = time.perf_counter()
        want_xyz = torch.from_numpy(np.ascontiguousarray(pcnp)).to(dev)
        want_cls = torch.from_numpy(classes).to(dev)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        host_ms.append((t1 - t0) * 1e3)
        upload_ms.append((t2 - t1) * 1e3)

    # (a) the kernel alone, on two buffer sets of n * (S + 32) bytes each, the records at an odd address
    sets = []
    for _ in range(2):
        raw = torch.empty(n * S + 16, dtype=torch.uint8, device=dev)
        view = raw[1:1 + n * S]
        view.copy_(torch.from_numpy(rows.reshape(-1)))
        sets.append((view, torch.empty((n, 3), dtype=torch.float64, device=dev),
                     torch.empty((n,), dtype=torch.float64, device=dev), torch.zeros(256, dtype=torch.int64, device=dev)))
    calls = [lambda s=s: _hip.las_decode(s[0], n, fmt, S, SCALE, OFFSET, s[1], s[2], s[3]) for s in sets]
    calls[0]()
    torch.cuda.synchronize()
    assert torch.equal(sets[0][1].view(torch.int64), want_xyz.view(torch.int64)), "decode differs from the host baseline"
    assert torch.equal(sets[0][2], want_cls.to(torch.float64))
    assert torch.equal(sets[0][3], torch.bincount(want_cls.to(torch.int64), minlength=256))
    decode_us = per_call_us(calls, iters)
    del sets, calls
    med = statistics.median(decode_us)
    yard = statistics.median(unpack_us) * (S + 32) / 64

    # (b) the reader, page cache warm
    scan = reader.read(path)
    torch.cuda.synchronize()
    assert torch.equal(scan.xyz.view(torch.int64), want_xyz.view(torch.int64)) and torch.equal(scan.classes, want_cls.to(torch.float64))
    read_ms = []
    for _ in range(5):
        del scan
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        scan = reader.read(path)
        torch.cuda.synchronize()
        read_ms.append((time.perf_counter() - t0) * 1e3)
    file_bytes = n * S
    res = {"format": fmt, "record_length": S, "points": n, "data_offset": off,
           "decode_us": spread(decode_us), "bytes_per_point": S + 32,
           "decode_bytes_per_s": round(n * (S + 32) / (med * 1e-6), 0), "decode_hbm_share": round(n * (S + 32) / (med * 1e-6) / HBM_PEAK, 3),
           "yardstick_us": round(yard, 2), "decode_over_yardstick": round(med / yard, 3), "margin": MARGIN,
           "within_margin": bool(med <= MARGIN * yard),
           "reader_ms": spread(read_ms), "reader_file_bytes_per_s": round(file_bytes / (statistics.median(read_ms) * 1e-3), 0),
           "host_decode_ms": spread(host_ms), "host_upload_ms": spread(upload_ms),
           "host_over_reader": round((statistics.median(host_ms) + statistics.median(upload_ms)) / statistics.median(read_ms), 2)}
    print(f"format {fmt} ({S} B): decode {res['decode_us']['median']:8.1f} us [{res['decode_us']['min']:.1f}, "
          f"{res['decode_us']['max']:.1f}] = {res['decode_hbm_share']:.2f} of HBM peak, / yardstick {res['decode_over_yardstick']:.2f}; "
          f"reader {res['reader_ms']['median']:7.1f} ms = {res['reader_file_bytes_per_s'] / 1e9:.2f} GB/s; host decode "
          f"{res['host_decode_ms']['median']:7.1f} ms + upload {res['host_upload_ms']['median']:6.1f} ms", flush=True)
    os.remove(path)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="las_bench.json")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--tmp", default=None, help="directory for the synthetic files (default: a temporary one)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("las_bench needs a HIP device (there is no CPU path)")
    dev = torch.device("cuda:0")
    n = args.points
    reader = LasReader(dev)

    # K7 on the same n, two buffer sets of 64 B per point each
    sets = [(torch.rand((n, 4), dtype=torch.float64, device=dev), torch.empty((n, 3), dtype=torch.float64, device=dev),
             torch.empty((n,), dtype=torch.float64, device=dev)) for _ in range(2)]
    unpack_us = per_call_us([lambda s=s: _hip.tiles_unpack(s[0], s[1], s[2]) for s in sets], args.iters)
    del sets

    # a pinned host-to-device copy of one chunk of the reader's size
    chunk = reader.chunk_bytes
    host, raw = torch.empty(chunk, dtype=torch.uint8).pin_memory(), torch.empty(chunk, dtype=torch.uint8, device=dev)
    h2d_us = per_call_us([lambda: raw.copy_(host, non_blocking=True)], args.iters)
    del host, raw
    h2d_rate = chunk / (statistics.median(h2d_us) * 1e-6)

    res = {"device": torch.cuda.get_device_name(dev), "points": n, "chunk_records": _hip.las_chunk_records(),
           "hbm_peak_bytes_per_s": HBM_PEAK, "tiles_unpack_us": spread(unpack_us),
           "tiles_unpack_hbm_share": round(n * 64 / (statistics.median(unpack_us) * 1e-6) / HBM_PEAK, 3),
           "pinned_h2d_chunk_bytes": chunk, "pinned_h2d_us": spread(h2d_us), "pinned_h2d_bytes_per_s": round(h2d_rate, 0),
           "yardstick": "sn_tiles_unpack (f64, 4 columns, same n) in the same run, times (S + 32) / 64; margin 1.25",
           "host_baseline": "numpy structured decode + vstack().transpose() + upload; stands in for laspy, which is not installed",
           "cases": []}
    print(f"sn_tiles_unpack {res['tiles_unpack_us']['median']:.1f} us [{res['tiles_unpack_us']['min']:.1f}, "
          f"{res['tiles_unpack_us']['max']:.1f}] = {res['tiles_unpack_hbm_share']:.2f} of HBM peak; pinned H2D "
          f"{h2d_rate / 1e9:.1f} GB/s", flush=True)
    with tempfile.TemporaryDirectory(dir=args.tmp) as tmp:
        for fmt in (1, 3, 6):
            case = bench_format(fmt, n, args.iters, tmp, dev, reader, unpack_us)
            case["reader_share_of_pinned_h2d"] = round(case["reader_file_bytes_per_s"] / h2d_rate, 3)
            res["cases"].append(case)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
