#!/usr/bin/env python3
"""The z-walk's job plan and its dead jobs (csrc/conv_i8s.hip where ZShape is filled, csrc/conv_i8z.inc "DEAD JOBS") restated
in numpy, with the cost model the dealt two-segment plan was chosen by.  No GPU.

A job is (tile b, 8 x-rows from x0, 64 y from y0, LZ output planes from zs).  It is DEAD when no voxel of tile b is set in
planes zs - 4 .. zs + LZ + 3, rows x0 - 4 .. x0 + 11, y0 - 4 .. y0 + 67 (clipped to the grid): the union of the windows of
all its rounds under the kernel's conservative row rule (tools/debug/zwalk_window_rule.py), so none of its rounds would run.
A workgroup of the head-only launch fills its dead jobs and walks the live ones.

  plan(B, Z, X, Y, segments, ...)   -> the launch's plan as the host forms it (segments as option conv_i8z_segments)
  jobs(p)                           -> per workgroup, its jobs (b, x0, y0, zs) in the kernel's numbering
  live(occ, p, job)                 -> the rule above
  run_map(occ, kH)                  -> which rounds the window rule runs, per (y tile, b, z, round of the tile's rows)
  job_rounds(runs, p, job, kH)      -> rounds of one job that run
  cost(occ, p, kH)                  -> modelled microseconds per workgroup
  python tools/debug/zwalk_plan_model.py    the benchmark's batch (32 synthetic tiles, 100 k points, 64^3): the parent's plan
                                            and the dealt two-segment plan, max / median / mean over the workgroups"""
import os
import sys

import numpy as np

K_ZTX, K_TY, K_MAX_JOBS, K_ZD = 8, 64, 256, 11
# workgroup time = PROLOGUE + PLANE x (planes streamed) + ROUND x (rounds run), microseconds: the prologue as measured, an
# all-zero batch 40.6 us over 72 planes, conv_i8z_dense = 1 103 us over 512 rounds
T_PROLOGUE, T_PLANE, T_ROUND = 3.2, 0.52, 0.122


def plan(B, Z, X, Y, segments=0, cus=256, head_only=True, dense=False):
    """segments: 1 = the dense walk's plan, n >= 2 = n dealt segments where the guards allow, 0 = auto"""
    nxt, nyt = (X + K_ZTX - 1) // K_ZTX, (Y + K_TY - 1) // K_TY
    ncol = B * nxt * nyt
    best_seg, best_cost, max_seg = 1, -1, (Z + 7) // 8
    for ns in range(1, max_seg + 1):
        lz = (Z + ns - 1) // ns
        per_wg = (ncol * ((Z + lz - 1) // lz) + cus - 1) // cus
        if per_wg > K_MAX_JOBS:
            continue
        c = per_wg * (lz + 8) + K_ZD
        if best_cost < 0 or c < best_cost:
            best_cost, best_seg = c, ns
    assert best_cost >= 0
    deal, shift = 0, 0
    if not dense:
        n = segments if segments >= 2 else (2 if segments == 0 and head_only and nxt >= 2 and Z >= 32 and best_seg == 1 else 0)
        if 2 <= n <= max_seg and (ncol * n + cus - 1) // cus <= K_MAX_JOBS:
            best_seg, deal, shift = n, 1, max(1, nxt // n)
    LZ = (Z + best_seg - 1) // best_seg
    nseg = (Z + LZ - 1) // LZ
    njobs = ncol * nseg
    grid = min(njobs, cus)
    return dict(B=B, Z=Z, X=X, Y=Y, nxt=nxt, nyt=nyt, ncol=ncol, LZ=LZ, PL=LZ + 8, nseg=nseg, njobs=njobs, grid=grid,
                swizzle=int(grid % 8 == 0), deal=deal, shift=shift, fill_dead=int(bool(deal) and head_only))


def job_id(p, wg, k):
    """zjob_id: job k of workgroup wg, with the XCD swizzle on the full rounds of the grid"""
    base, grid = k * p["grid"], p["grid"]
    if p["swizzle"] and base + grid <= p["njobs"]:
        return base + (wg & 7) * (grid >> 3) + (wg >> 3)
    return base + wg


def decode(p, j):
    """job number -> (b, x0, y0, zs), and (b, yt, xt, sg)"""
    if p["deal"]:
        sg, j = divmod(j, p["ncol"])
        j, xt = divmod(j, p["nxt"])
        b, yt = divmod(j, p["nyt"])
        xt = (xt + p["shift"] * sg) % p["nxt"]
    else:
        j, xt = divmod(j, p["nxt"])
        j, yt = divmod(j, p["nyt"])
        b, sg = divmod(j, p["nseg"])
    return (b, xt * K_ZTX, yt * K_TY, sg * p["LZ"]), (b, yt, xt, sg)


def jobs(p):
    out = []
    for wg in range(p["grid"]):
        n = (p["njobs"] - 1 - wg) // p["grid"] + 1 if wg < p["njobs"] else 0
        out.append([decode(p, job_id(p, wg, k))[0] for k in range(n)])
    return out


def region(p, job):
    """the operand region of a job, clipped: slices (z, x, y)"""
    b, x0, y0, zs = job
    return (b, slice(max(0, zs - 4), min(p["Z"], zs + p["LZ"] + 4)), slice(max(0, x0 - 4), min(p["X"], x0 + 12)),
            slice(max(0, y0 - 4), min(p["Y"], y0 + 68)))


def live(occ, p, job):
    return bool(occ[region(p, job)].any())


def run_map(occ, kH=1):
    """[nyt][B, Z, rounds over all x tiles] bool: the window rule's verdict per round (the restatement of
    zwalk_window_rule._count that keeps the map; its sums are that function's)"""
    occ = np.asarray(occ).astype(bool)
    B, Z, X, Y = occ.shape
    maps = []
    for yt in range((Y + 63) // 64):
        y0 = 64 * yt
        rows = occ[..., max(0, y0 - 4):min(Y, y0 + 68)].any(axis=-1)
        pad = np.zeros((B, Z + 8, X + 16), dtype=bool)
        pad[:, 4:4 + Z, 4:4 + X] = rows
        zwin = np.zeros((B, Z, X + 16), dtype=bool)
        for dz in range(9):
            zwin |= pad[:, dz:dz + Z]
        per_x = {}
        for xt in range((X + 7) // 8):
            x0 = 8 * xt
            for h in range(0, min(8, X - x0), kH):
                per_x[(xt, h)] = zwin[:, :, x0 + h:x0 + h + kH + 8].any(axis=-1)
        maps.append(per_x)
    return maps


def job_rounds(runs, p, job, kH=1):
    """(rounds of the job that run, rounds it has)"""
    b, x0, y0, zs = job
    z1 = min(p["Z"], zs + p["LZ"])
    ran = total = 0
    for h in range(0, min(8, p["X"] - x0), kH):
        m = runs[y0 // 64][(x0 // 8, h)][b, zs:z1]
        ran += int(m.sum())
        total += m.size
    return ran, total


def cost(occ, p, kH=1):
    """modelled microseconds per workgroup; a dead job of a fill_dead plan streams no plane"""
    runs = run_map(occ, kH)
    t = []
    for mine in jobs(p):
        planes = rounds = 0
        for job in mine:
            if p["fill_dead"] and not live(occ, p, job):
                continue
            planes += p["PL"]
            rounds += job_rounds(runs, p, job, kH)[0]
        t.append(T_PROLOGUE + T_PLANE * planes + T_ROUND * rounds)
    return np.array(t)


def main():
    root = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.path.insert(0, root)
    from oracle import voxel_oracle as vo
    from scene_net_amd.synthetic import synthetic_tile
    occ = np.zeros((32, 64, 64, 64), dtype=bool)
    for t in range(32):
        c, _, _ = vo.voxel_counts(synthetic_tile(t, 100_000)[0], (64, 64, 64), None, None, None)
        occ[t] = (vo.to_full_dense(vo.normalize_xyz(c.astype(np.float64))) > 0).reshape(64, 64, 64)
    for name, seg in (("whole columns (conv_i8z_segments = 1)", 1), ("two dealt segments (auto)", 0)):
        p = plan(32, 64, 64, 64, seg)
        dead = sum(not live(occ, p, j) for mine in jobs(p) for j in mine) if p["fill_dead"] else 0
        t = cost(occ, p, 1)
        print(f"{name}: {p['njobs']} jobs, {dead} dead, shift {p['shift']}; workgroup us max {t.max():.1f} "
              f"median {np.median(t):.1f} mean {t.mean():.1f}")


if __name__ == "__main__":
    main()
