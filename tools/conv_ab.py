#!/usr/bin/env python3
"""A/B of the three forms of K3' (folded kernel vs stride-4 kernel vs four-copy kernel) and of the guard's gated fp32 launch, interleaved
rounds in ONE process on the bench's C2 batch (cdna_hip_programming.md rule 24).
    python tools/conv_ab.py [--rounds 5] [--iters 40] [--batch 32] [--grid 64]
    python tools/conv_ab.py --skip      the z-walk with and without its empty-window skip (sn_set_option "conv_i8z_dense"),
                                        a dense / skip pair of rows on the C2 batch, on random 50 % occupancy (no window is
                                        empty: the price of the check) and on an all-zero batch (the floor of a launch that
                                        skips every round), with the rounds run / skipped of one launch
    python tools/conv_ab.py --skip --bits   the same three inputs through sn_conv_bank_prepared_rows: without row bits (the
                                        static two-segment deal and its byte check), with bits and two segments, with bits
                                        and four (the default with bits at Z = 64): the balanced deal, conv_i8z.inc
    python tools/conv_ab.py --skip --bits --trim   ... and the two rows with bits once more under conv_i8z_trim = 0 (every live
                                        job streamed whole), with the planes one launch streamed / trimmed away: on random
                                        50 % and on all zero nothing can be trimmed -- those pairs price the cursor"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import scene_net_amd as sna  # noqa: E402
from scene_net_amd import _hip  # noqa: E402
from scene_net_amd.synthetic import apply_bank_spec, synthetic_bank_spec, synthetic_tile  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--grid", type=int, default=64)
    ap.add_argument("--points", type=int, default=100_000)
    ap.add_argument("--random-occ", type=float, default=0.0, help="random occupancy of this density instead of tiles")
    ap.add_argument("--skip", action="store_true", help="dense / skip rows of the z-walk on three inputs")
    ap.add_argument("--bits", action="store_true", help="with --skip: hand the occupancy's row bits to the walk")
    ap.add_argument("--trim", action="store_true", help="with --skip --bits: rows under conv_i8z_trim = 0 beside the default")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    specs, names, lambdas, last = synthetic_bank_spec()
    torch.manual_seed(0)
    model = sna.SceneNet({"cy": 6, "cone": 5, "neg": 5}, (9, 9, 9))
    apply_bank_spec(model, specs, names, lambdas, last)
    model = model.to(dev)
    bank, lam = model.compute_bank(dev), model.effective_lambdas(dev)
    if args.random_occ > 0:
        occ = torch.rand((args.batch, 1) + (args.grid,) * 3, device=dev) < args.random_occ
    else:
        tiles = [synthetic_tile(i, args.points)[0] for i in range(args.batch)]
        occ = sna.voxelize_batch(sna.PointBatch.from_tiles(tiles, device=dev), (args.grid,) * 3,
                                 occ_dtype=torch.bool).occ

    prep = _hip.conv_bank_prep(bank)
    if args.skip and args.bits:
        return bits_ab(args, occ, bank, lam, prep)
    if args.skip:
        return skip_ab(args, occ, bank, lam, prep)
    use_prep = [False]

    def run(n):
        for _ in range(n):
            _hip.conv_bank(occ, bank, lam, want_act=False, want_out=True, prep=prep if use_prep[0] else None)

    variants = {
        "zwalk 2x1x8+guard": dict(legacy=0, tol=90000, fold=1, prep=True, zv=0),
        "zwalk 1x1x12+guard": dict(legacy=0, tol=90000, fold=1, prep=True, zv=1),
        "zwalk 1x2x12+guard": dict(legacy=0, tol=90000, fold=1, prep=True, zv=2),
        "zwalk 1x2x12 noguard": dict(legacy=0, tol=0, fold=1, prep=True, zv=2),
        "folded+guard": dict(legacy=0, tol=90000, fold=1),
        "folded noguard": dict(legacy=0, tol=0, fold=1),
        "stride4+guard": dict(legacy=0, tol=90000, fold=0),
        "stride4 noguard": dict(legacy=0, tol=0, fold=0),
        "legacy+guard": dict(legacy=1, tol=90000, fold=0),
        "legacy noguard": dict(legacy=1, tol=0, fold=0),
    }
    for k, v in os.environ.items():
        if k.startswith("SN_CONV"):
            print("env", k, v)
    res = {k: [] for k in variants}
    t_spin = time.perf_counter()
    while time.perf_counter() - t_spin < 0.3:
        run(10)
        torch.cuda.synchronize()
    for r in range(args.rounds):
        for name, v in variants.items():
            _hip.set_option("conv_i8_legacy", v["legacy"])
            _hip.set_option("conv_i8_tolerance_ppb", v["tol"])
            _hip.set_option("conv_i8_fold", v["fold"])
            use_prep[0] = bool(v.get("prep"))
            if "zv" in v:
                _hip.set_option("conv_i8z_variant", v["zv"])
            run(5)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run(args.iters)
            e1.record()
            torch.cuda.synchronize()
            res[name].append(e0.elapsed_time(e1) / args.iters)
    _hip.set_option("conv_i8_legacy", 0)
    _hip.set_option("conv_i8_tolerance_ppb", 90000)
    _hip.set_option("conv_i8_fold", 1)
    flops = 2.0 * args.grid ** 3 * 729 * 16 * args.batch
    for name, ts in res.items():
        med, mn = float(np.median(ts)), float(np.min(ts))
        print(f"{name:18s} median {med * 1e3:8.1f} us  min {mn * 1e3:8.1f} us  {flops / (med * 1e-3) / 1e12:7.1f} TFLOP/s "
              f"algorithmic  rounds {[round(t * 1e3, 1) for t in ts]}")


def skip_ab(args, tiles_occ, bank, lam, prep):
    """the prepared, served z-walk (what bench.py's step runs) with conv_i8z_dense = 1 and 0, interleaved"""
    g = torch.Generator(device=tiles_occ.device).manual_seed(1)
    inputs = {"C2 batch": tiles_occ,
              "random 50 %": torch.rand(tiles_occ.shape, device=tiles_occ.device, generator=g) < 0.5,
              "all zero": torch.zeros_like(tiles_occ)}
    out = torch.empty(tiles_occ.shape, dtype=torch.float32, device=tiles_occ.device)
    fn = _hip.load().sn_conv_bank_prepared_served
    B, _, Z, X, Y = tiles_occ.shape
    G = bank.shape[0]
    stream = torch.cuda.current_stream().cuda_stream

    def run(x, n):
        for _ in range(n):
            rc = fn(x.data_ptr(), _hip.SN_OCC8, bank.data_ptr(), lam.data_ptr(), prep.data_ptr(), B, Z, X, Y, G, 9, 9, 9, None,
                    out.data_ptr(), _hip.SN_F32, stream)
            assert rc == 0, rc

    rows = [(name, dense) for name in inputs for dense in (1, 0)]
    res = {r: [] for r in rows}
    counts, kept = {}, {}
    t_spin = time.perf_counter()
    while time.perf_counter() - t_spin < 0.3:
        run(tiles_occ, 10)
        torch.cuda.synchronize()
    for r in range(args.rounds):
        for name, dense in rows:
            _hip.set_option("conv_i8z_dense", dense)
            run(inputs[name], 5)
            torch.cuda.synchronize()
            if r == 0:
                c0 = _hip.conv_i8z_round_counts()
                run(inputs[name], 1)
                c1 = _hip.conv_i8z_round_counts()
                counts[(name, dense)] = (c1[0] - c0[0], c1[1] - c0[1])
                kept[(name, dense)] = out.clone()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run(inputs[name], args.iters)
            e1.record()
            torch.cuda.synchronize()
            res[(name, dense)].append(e0.elapsed_time(e1) / args.iters)
    _hip.set_option("conv_i8z_dense", 0)
    for name, dense in rows:
        ts = res[(name, dense)]
        ran, skipped = counts[(name, dense)]
        same = torch.equal(kept[(name, 0)].view(torch.int32), kept[(name, 1)].view(torch.int32))
        print(f"{name:12s} {'dense' if dense else 'skip ':5s} median {float(np.median(ts)) * 1e3:8.1f} us  min {float(np.min(ts)) * 1e3:8.1f} us  "
              f"rounds run {ran} skipped {skipped} ({100.0 * ran / max(1, ran + skipped):5.1f} % run)  same bits {same}  "
              f"rounds {[round(t * 1e3, 1) for t in ts]}")
    print(f"spin give-ups {_hip.conv_i8_spin_timeouts()}, device status {_hip.device_status()[0]}")


def bits_ab(args, tiles_occ, bank, lam, prep):
    """the prepared, served z-walk without row bits, with bits and two segments, with bits and four, interleaved"""
    g = torch.Generator(device=tiles_occ.device).manual_seed(1)
    inputs = {"C2 batch": tiles_occ,
              "random 50 %": torch.rand(tiles_occ.shape, device=tiles_occ.device, generator=g) < 0.5,
              "all zero": torch.zeros_like(tiles_occ)}
    bits = {name: _hip.row_bits_of(x) for name, x in inputs.items()}
    out = torch.empty(tiles_occ.shape, dtype=torch.float32, device=tiles_occ.device)
    fn = _hip.load().sn_conv_bank_prepared_rows
    B, _, Z, X, Y = tiles_occ.shape
    G = bank.shape[0]
    stream = torch.cuda.current_stream().cuda_stream
    modes = {"no bits": (False, 0, 1), "bits, 2 segments": (True, 2, 1), "bits, 4 segments": (True, 4, 1)}
    if args.trim:
        modes.update({"bits, 2, untrimmed": (True, 2, 0), "bits, 4, untrimmed": (True, 4, 0)})

    def run(name, mode, n):
        with_bits, seg, trim = modes[mode]
        _hip.set_option("conv_i8z_segments", seg)
        _hip.set_option("conv_i8z_trim", trim)
        for _ in range(n):
            rc = fn(inputs[name].data_ptr(), _hip.SN_OCC8, bank.data_ptr(), lam.data_ptr(), prep.data_ptr(), B, Z, X, Y, G, 9, 9,
                    9, None, out.data_ptr(), _hip.SN_F32, stream, 1, bits[name].data_ptr() if with_bits else None, None)
            assert rc == 0, rc

    rows = [(name, mode) for name in inputs for mode in modes]
    res = {r: [] for r in rows}
    kept, planes = {}, {}
    t_spin = time.perf_counter()
    while time.perf_counter() - t_spin < 0.3:
        run("C2 batch", "no bits", 10)
        torch.cuda.synchronize()
    for r in range(args.rounds):
        for name, mode in rows:
            run(name, mode, 5)
            torch.cuda.synchronize()
            if r == 0:
                p0 = _hip.conv_i8z_plane_counts()
                run(name, mode, 1)
                p1 = _hip.conv_i8z_plane_counts()
                planes[(name, mode)] = (p1[0] - p0[0], p1[1] - p0[1])
                kept[(name, mode)] = out.clone()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run(name, mode, args.iters)
            e1.record()
            torch.cuda.synchronize()
            res[(name, mode)].append(e0.elapsed_time(e1) / args.iters)
    _hip.set_option("conv_i8z_segments", 0)
    _hip.set_option("conv_i8z_trim", 1)
    for name, mode in rows:
        ts = res[(name, mode)]
        same = torch.equal(kept[(name, mode)].view(torch.int32), kept[(name, "no bits")].view(torch.int32))
        print(f"{name:12s} {mode:18s} median {float(np.median(ts)) * 1e3:8.1f} us  min {float(np.min(ts)) * 1e3:8.1f} us  "
              f"same bits {same}  planes streamed {planes[(name, mode)][0]} trimmed {planes[(name, mode)][1]}  rounds {[round(t * 1e3, 1) for t in ts]}")
    print(f"spin give-ups {_hip.conv_i8_spin_timeouts()}, device status {_hip.device_status()[0]}")


if __name__ == "__main__":
    main()
