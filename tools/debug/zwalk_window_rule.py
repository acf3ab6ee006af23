#!/usr/bin/env python3
"""The z-walk's empty-window rule (csrc/conv_i8z.inc, header comment "EMPTY WINDOWS") restated in numpy: which rounds of a
launch the kernel runs and which it skips, from the occupancy alone.  No GPU.

A column is (tile b, 8 x-rows from x0 = 8 xt, 64 y from y0 = 64 yt).  The fold pass marks halo row r (grid row x0 - 4 + r,
r = 0..15) of grid plane z NON-EMPTY when any voxel (z, x0 - 4 + r, y) with y0 - 4 <= y < y0 + 68 inside the grid is set --
the bytes its 16 lanes read.  A round covers kH x-rows h .. h + kH - 1 of the column on one output plane z (kH = 2 for
conv_i8z_variant 0, else 1); it runs when any of the halo rows h .. h + kH + 7 of the planes z - 4 .. z + 4 is non-empty, i.e.
when a set voxel lies within |dz| <= 4, |dx| <= 4 of one of its rows AND inside the column's y extent +- 4 (+ 4 more on the
high side when the column's last lanes read on: the rule is per row, not per output).  Rounds exist for rows and planes
inside the grid only.

  counts(occ, kH)        -> (rounds run, rounds skipped) under the kernel's rule
  counts_exact(occ, kH)  -> the same with the exact window of each round's own outputs (y0 - 4 .. y0 + Yt + 3): a lower
                            bound of the rounds run
  python tools/debug/zwalk_window_rule.py    the benchmark's batch (32 synthetic tiles, 100 k points, 64^3)"""
import os
import sys

import numpy as np


def _row_any(occ, y_lo, y_hi):
    """occ [B, Z, X, Y] bool -> [B, Z, X]: a set voxel with y_lo <= y < y_hi (clipped to the grid)"""
    Y = occ.shape[-1]
    lo, hi = max(0, y_lo), min(Y, y_hi)
    if lo >= hi:
        return np.zeros(occ.shape[:-1], dtype=bool)
    return occ[..., lo:hi].any(axis=-1)


def _count(occ, kH, exact):
    occ = np.asarray(occ).astype(bool)
    if occ.ndim == 5:
        occ = occ[:, 0]
    B, Z, X, Y = occ.shape
    ran = skipped = 0
    for yt in range((Y + 63) // 64):
        y0 = 64 * yt
        ny = min(64, Y - y0)
        rows = _row_any(occ, y0 - 4, y0 + (ny + 4 if exact else 68))          # [B, Z, X]
        # a set row within |dz| <= 4 of plane z: dilate along z
        pad = np.zeros((B, Z + 8, X + 8 + 8), dtype=bool)                      # x padded by 4 below and 4 + 8 above
        pad[:, 4:4 + Z, 4:4 + X] = rows
        zwin = np.zeros((B, Z, X + 16), dtype=bool)
        for dz in range(9):
            zwin |= pad[:, dz:dz + Z]
        for xt in range((X + 7) // 8):
            x0 = 8 * xt
            nrows = min(8, X - x0)
            for h in range(0, nrows, kH):
                # halo rows h .. h + kH + 7 of the column = grid rows x0 - 4 + h ..: padded index x0 + h ..
                hit = zwin[:, :, x0 + h:x0 + h + kH + 8].any(axis=-1)           # [B, Z]
                ran += int(hit.sum())
                skipped += int((~hit).sum())
    return ran, skipped


def counts(occ, kH=1):
    return _count(occ, kH, exact=False)


def counts_exact(occ, kH=1):
    return _count(occ, kH, exact=True)


def main():
    root = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.path.insert(0, root)
    from oracle import voxel_oracle as vo
    from scene_net_amd.synthetic import synthetic_tile
    tot = [0, 0]
    for t in range(32):
        c, _, _ = vo.voxel_counts(synthetic_tile(t, 100_000)[0], (64, 64, 64), None, None, None)
        occ = vo.to_full_dense(vo.normalize_xyz(c.astype(np.float64))) > 0
        r, s = counts(occ[None], 1)
        tot[0] += r
        tot[1] += s
        print(f"tile {t:2d}: occupancy {occ.mean() * 100:5.2f} %, rounds run {r} skipped {s} ({100.0 * r / (r + s):.1f} % run)")
    print(f"batch: rounds run {tot[0]} skipped {tot[1]} ({100.0 * tot[0] / (tot[0] + tot[1]):.1f} % run)")


if __name__ == "__main__":
    main()
