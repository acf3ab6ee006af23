#!/usr/bin/env python3
"""K15 LAS encode on synthetic scans of 10^7 points in the point formats 1 (28 B), 3 (34 B) and 6 (30 B), every optional
array the format has present.  Everything is measured in this one run, after a warm-up, per call between HIP events
(kernels, copies) or by the host clock around work that ends in a synchronise (files); reported as the median with the
minimum and the maximum:
  (a) sn_las_encode alone, rotating over buffer sets so that no call finds its bytes in the 256 MiB last-level cache; next
      to it sn_las_decode (K13) of the records just written, on rotated buffers in the same run.  That is the yardstick: the
      same bytes move the other way.  The encode is meant to stay within 25 % of it.  A reported figure, not an assertion.
  (b) LasWriter.write of the scan to a file on a RAM-backed path: total time, and file bytes per second against the rate
      of a pinned device-to-host copy of one chunk measured here, and against the rate at which the host thread alone
      writes pinned bytes into a fresh file of the same directory.
  (c) the host baseline: the download of xyz and classes, then numpy's np.rint((x - offset) / scale) per column, the fields
      assigned to the structured record array and tofile -- tests/las_write_cases.encode_oracle.  It stands in for laspy's
      assignment and write; laspy itself is not installed where this runs.
The bench checks what it times against (c)'s bytes, byte for byte.  One JSON file.
    python tools/las_write_bench.py --out profiles/las_write_bench.json [--points 10000000] [--iters 20]"""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
from scene_net_amd import _hip  # noqa: E402
from scene_net_amd.las import LAS_STANDARD_LENGTH  # noqa: E402
from scene_net_amd.las_write import LasWriter  # noqa: E402
import las_write_cases as wc  # noqa: E402

HBM_PEAK = 8.0e12      # bytes / s, the part's specification
MARGIN = 1.25
SCALE, OFFSET = (0.01, 0.01, 0.01), (5.0e5, 4.6e6, 100.0)
# a TS40K-like class mix: a few classes carry nearly all points, which is what the LDS histogram has to live with
CLASSES, CLASS_P = np.array([2, 3, 4, 5, 1, 14, 15, 16], dtype=np.float64), [.38, .2, .15, .2, .04, .015, .005, .01]


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


def synthetic_scan(n, fmt, seed=0):
    """a scan 2 km x 2 km x 60 m on the centimetre grid's neighbourhood, the class mix above, every optional array"""
    rng = np.random.default_rng(seed + fmt)
    xyz = rng.uniform(0.0, 1.0, (n, 3)) * np.array([2000.0, 2000.0, 60.0]) + np.array(OFFSET)
    inp = {"xyz": xyz, "classes": rng.choice(CLASSES, size=n, p=CLASS_P),
           "intensity": rng.integers(0, 65536, n).astype(np.uint16), "gps": rng.uniform(0.0, 6.0e5, n), "rgb": None}
    if fmt in wc.RGB_FORMATS:
        inp["rgb"] = rng.integers(0, 65536, (n, 3)).astype(np.uint16)
    return inp


def bench_format(fmt, n, iters, tmp, dev, writer):
    S = LAS_STANDARD_LENGTH[fmt]
    inp = synthetic_scan(n, fmt)
    t = {k: (None if v is None else torch.from_numpy(v).to(dev)) for k, v in inp.items()}
    in_bytes = 24 + 8 + 2 + 8 + (6 if inp["rgb"] is not None else 0)

    # (c) the host baseline (also the reference bytes of this scan): download, encode, tofile
    host_ms, download_ms = [], []
    path = os.path.join(tmp, f"host{fmt}.las")
    for _ in range(2):
        t0 = time.perf_counter()
        xyz_h, cls_h = t["xyz"].cpu().numpy(), t["classes"].cpu().numpy()
        t1 = time.perf_counter()
        rows, box, hist, bad = wc.encode_oracle(xyz_h, cls_h, inp["intensity"], inp["gps"], inp["rgb"], fmt, 0, SCALE, OFFSET)
        with open(path, "wb") as f:
            rows.tofile(f)
        t2 = time.perf_counter()
        download_ms.append((t1 - t0) * 1e3)
        host_ms.append((t2 - t1) * 1e3)
    os.remove(path)
    assert bad == (0, 0)
    want = torch.from_numpy(rows.reshape(-1)).to(dev)

    # (a) the kernel alone, on two buffer sets; then K13's decode of what it wrote
    sets = []
    for k in range(2):
        ins = t if k == 0 else {key: (None if v is None else v.clone()) for key, v in t.items()}
        sets.append((ins, torch.empty(n * S, dtype=torch.uint8, device=dev), torch.tensor(wc.EMPTY_BOX, dtype=torch.int32, device=dev),
                     torch.zeros(256, dtype=torch.int64, device=dev), torch.zeros(2, dtype=torch.int64, device=dev)))
    calls = [lambda s=s: _hip.las_encode(s[0]["xyz"], n, fmt, S, SCALE, OFFSET, s[1], s[0]["classes"], s[0]["intensity"],
                                         s[0]["gps"], s[0]["rgb"], s[2], s[3], s[4]) for s in sets]
    for c in calls:
        c()
    torch.cuda.synchronize()
    for s in sets:
        assert torch.equal(s[1], want), "encode differs from the host baseline"
    assert tuple(sets[0][2].tolist()) == box and np.array_equal(sets[0][3].cpu().numpy(), hist) and sets[0][4].tolist() == [0, 0]
    encode_us = per_call_us(calls, iters)
    outs = [(torch.empty((n, 3), dtype=torch.float64, device=dev), torch.empty((n,), dtype=torch.float64, device=dev),
             torch.zeros(256, dtype=torch.int64, device=dev)) for _ in range(2)]
    dcalls = [lambda s=s, o=o: _hip.las_decode(s[1], n, fmt, S, SCALE, OFFSET, o[0], o[1], o[2]) for s, o in zip(sets, outs)]
    decode_us = per_call_us(dcalls, iters)
    assert torch.equal(outs[0][1], t["classes"]), "decode of the written records gives other classes"
    del sets, calls, outs, dcalls, want
    enc, dec = statistics.median(encode_us), statistics.median(decode_us)

    # (b) the writer, to a RAM-backed file
    path = os.path.join(tmp, f"format{fmt}.las")
    head = writer.write(path, t["xyz"], t["classes"], t["intensity"], t["gps"], t["rgb"], point_format=fmt, scale=SCALE,
                        offset=OFFSET)
    assert head.n_points == n and head.box == box and head.bad == (0, 0)
    with open(path, "rb") as f:
        f.seek(head.data_offset)
        assert f.read() == rows.tobytes(), "the written file differs from the host baseline"
    write_ms = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        writer.write(path, t["xyz"], t["classes"], t["intensity"], t["gps"], t["rgb"], point_format=fmt, scale=SCALE, offset=OFFSET)
        write_ms.append((time.perf_counter() - t0) * 1e3)
    os.remove(path)
    file_bytes = n * S
    res = {"format": fmt, "record_length": S, "points": n, "bytes_per_point": in_bytes + S,
           "encode_us": spread(encode_us), "encode_bytes_per_s": round(n * (in_bytes + S) / (enc * 1e-6), 0),
           "encode_hbm_share": round(n * (in_bytes + S) / (enc * 1e-6) / HBM_PEAK, 3),
           "decode_us": spread(decode_us), "decode_bytes_per_point": S + 32, "encode_over_decode": round(enc / dec, 3),
           "margin": MARGIN, "within_margin": bool(enc <= MARGIN * dec),
           "writer_ms": spread(write_ms), "writer_file_bytes_per_s": round(file_bytes / (statistics.median(write_ms) * 1e-3), 0),
           "host_download_ms": spread(download_ms), "host_encode_tofile_ms": spread(host_ms),
           "host_over_writer": round((statistics.median(host_ms) + statistics.median(download_ms)) / statistics.median(write_ms), 2)}
    print(f"format {fmt} ({S} B): encode {res['encode_us']['median']:8.1f} us [{res['encode_us']['min']:.1f}, "
          f"{res['encode_us']['max']:.1f}] = {res['encode_hbm_share']:.2f} of HBM peak, decode {res['decode_us']['median']:.1f} us, "
          f"ratio {res['encode_over_decode']:.2f}; writer {res['writer_ms']['median']:7.1f} ms = "
          f"{res['writer_file_bytes_per_s'] / 1e9:.2f} GB/s; host download {res['host_download_ms']['median']:6.1f} ms + encode "
          f"and tofile {res['host_encode_tofile_ms']['median']:7.1f} ms", flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="las_write_bench.json")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--tmp", default=None, help="directory for the files (default: /dev/shm when it exists: RAM-backed)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("las_write_bench needs a HIP device (there is no CPU path)")
    dev = torch.device("cuda:0")
    n = args.points
    writer = LasWriter(dev)
    base = args.tmp or ("/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else None)

    # a pinned device-to-host copy of one chunk of the writer's size
    chunk = writer.chunk_bytes
    host, raw = torch.empty(chunk, dtype=torch.uint8).pin_memory(), torch.empty(chunk, dtype=torch.uint8, device=dev)
    d2h_us = per_call_us([lambda: host.copy_(raw, non_blocking=True)], args.iters)
    d2h_rate = chunk / (statistics.median(d2h_us) * 1e-6)
    # the host thread alone: four chunks from the pinned buffer into a fresh file of the same directory, as the writer writes
    file_write_ms = []
    with tempfile.TemporaryDirectory(dir=base) as tmp:
        for _ in range(5):
            t0 = time.perf_counter()
            with open(os.path.join(tmp, "plain.bin"), "wb", buffering=0) as f:
                for _ in range(4):
                    f.write(memoryview(host.numpy()))
            file_write_ms.append((time.perf_counter() - t0) * 1e3)
            os.remove(os.path.join(tmp, "plain.bin"))
    file_write_rate = 4 * chunk / (statistics.median(file_write_ms) * 1e-3)
    del host, raw

    res = {"device": torch.cuda.get_device_name(dev), "points": n, "chunk_records": _hip.las_encode_chunk_records(),
           "hbm_peak_bytes_per_s": HBM_PEAK, "pinned_d2h_chunk_bytes": chunk, "pinned_d2h_us": spread(d2h_us),
           "pinned_d2h_bytes_per_s": round(d2h_rate, 0), "host_file_write_ms_per_4_chunks": spread(file_write_ms),
           "host_file_write_bytes_per_s": round(file_write_rate, 0), "file_directory": base or "the default temporary directory",
           "yardstick": "sn_las_decode of the records just written (same n, same format) in the same run; margin 1.25",
           "host_baseline": "download of xyz and classes + numpy rint((x - offset) / scale), structured assignment, tofile; "
                            "stands in for laspy, which is not installed",
           "cases": []}
    print(f"pinned D2H {d2h_rate / 1e9:.1f} GB/s; the host thread writes a fresh file at {file_write_rate / 1e9:.2f} GB/s", flush=True)
    with tempfile.TemporaryDirectory(dir=base) as tmp:
        for fmt in (1, 3, 6):
            case = bench_format(fmt, n, args.iters, tmp, dev, writer)
            case["writer_share_of_pinned_d2h"] = round(case["writer_file_bytes_per_s"] / d2h_rate, 3)
            case["writer_share_of_host_file_write"] = round(case["writer_file_bytes_per_s"] / file_write_rate, 3)
            res["cases"].append(case)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
