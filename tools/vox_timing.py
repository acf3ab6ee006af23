#!/usr/bin/env python3
"""Debug only: per-workgroup phase times of occ_onepass_kernel (K1) at C2, from the wall_clock64 stamps a
`make -B EXTRA=-DSN_CONV_TIMING` build records (100 MHz clock).

    python tools/vox_timing.py            the tile workgroups alone
    python tools/vox_timing.py --riders   with K2 riding in the launch's first grid rows: the riders' phases too, and the
                                          launch's span (first start to last end) with and without them, median of --reps
"""
import argparse, ctypes, os, sys
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import scene_net_amd as sna
from scene_net_amd import _hip
from scene_net_amd.synthetic import apply_bank_spec, synthetic_bank_spec, synthetic_tile
ap = argparse.ArgumentParser()
ap.add_argument("--riders", action="store_true")
ap.add_argument("--reps", type=int, default=25)
args = ap.parse_args()
dev = torch.device("cuda:0")
tiles = [synthetic_tile(i, 100_000)[0] for i in range(32)]
batch = sna.PointBatch.from_tiles(tiles, device=dev)
rider = None
if args.riders:
    geneo_num = {"cy": 6, "cone": 5, "neg": 5}
    specs, names, lambdas, last = synthetic_bank_spec(geneo_num)
    model = sna.SceneNet(geneo_num, (9, 9, 9))
    apply_bank_spec(model, specs, names, lambdas, last)
    rider = model.to(dev).bank_rider(dev)
us = lambda a: a / 100.0


def stamps(bank_rider):
    """one launch -> its stamps [workgroups, 8] (int64), workgroups in grid order"""
    sna.voxelize_batch(batch, (64, 64, 64), occ_dtype=torch.bool, bank_rider=bank_rider)
    buf = np.zeros(1024 * 8, dtype=np.uint64)
    _hip.load().sn_debug_vox_times(buf.ctypes.data_as(ctypes.c_void_p))   # (synchronises)
    return buf.reshape(1024, 8).astype(np.int64)


def span(t):
    t = t[t[:, 0] > 0]
    return us(t[:, 6:8].max() - t[:, 0].min())


def show(name, a):
    print(f"{name:34s} min {a.min():8.2f} med {np.median(a):8.2f} max {a.max():8.2f}")


for _ in range(50):
    stamps(rider)
nrider = 0
if rider is not None:
    nrider = 16 * ((rider[0].shape[0] + 15) // 16)          # riders are the first workgroups of the grid
    t = stamps(rider)
    r = t[:nrider]
    r = r[r[:, 7] > 0]
    t0 = t[t[:, 0] > 0][:, 0].min()
    print("rider workgroups", len(r))
    show("start (after the launch's first)", us(r[:, 0] - t0))
    for k, name in enumerate(["phase 0 -> 1", "phase 1 -> 2", "phase 2 -> 3", "phase 3 -> 4", "phase 4 -> 5",
                              "phase 5 -> 6", "phase 6 -> 7"]):
        show(name, us(r[:, k + 1] - r[:, k]))
    show("whole rider", us(r[:, 7] - r[:, 0]))
    with_r = [span(stamps(rider)) for _ in range(args.reps)]
    # (a launch without riders is 256 tile workgroups, stamps 0..6: the rows and the column beyond are an earlier launch's)
    without = [span(stamps(None)[:256, :7]) for _ in range(args.reps)]
    print(f"launch span with riders    med {np.median(with_r):7.2f} min {min(with_r):7.2f} max {max(with_r):7.2f} us")
    print(f"launch span without riders med {np.median(without):7.2f} min {min(without):7.2f} max {max(without):7.2f} us")
    print(f"gap (medians) {np.median(with_r) - np.median(without):6.2f} us")
    t = stamps(rider)[nrider:]
else:
    t = stamps(None)
t = t[t[:, 0] > 0][:256]
t0 = t[:, 0].min()
print("tile workgroups", len(t))
show("start (after the first)", us(t[:, 0] - t0))
show("points in registers + min/max", us(t[:, 1] - t[:, 0]))
show("publish", us(t[:, 2] - t[:, 1]))
show("wait for the tile's 16 tags", us(t[:, 3] - t[:, 2]))
show("boxes + descriptor", us(t[:, 4] - t[:, 3]))
show("binning out of registers", us(t[:, 5] - t[:, 4]))
show("bitmap write-out", us(t[:, 6] - t[:, 5]))
show("whole workgroup", us(t[:, 6] - t[:, 0]))
show("end (after the first start)", us(t[:, 6] - t0))
