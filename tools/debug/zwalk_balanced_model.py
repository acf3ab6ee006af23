#!/usr/bin/env python3
"""The z-walk's BALANCED DEAL (csrc/conv_i8z.inc "THE BALANCED DEAL", its guard in csrc/conv_i8s.hip) restated in numpy on
top of the plan model (zwalk_plan_model.py): the row bits, the guard, the integer cost and the deal, exactly as the device
forms them.  No GPU.

Row bits: rows[b][z][w], uint32, w < ceil(X / 32); bit x % 32 of word x / 32 is set iff occ[b, z, x, :] holds a set voxel.
A superset of the true bits is allowed (it costs time, never a result).

Guard (host): bits given, the head-only form, not dense, one y tile (Y <= 64), Z <= 64, X <= 64; the plan is a dealt one
(option conv_i8z_segments n >= 2, or 0 = auto); the launch has exactly one workgroup per column (B ceil(X / 8) = compute
units: then the nxt workgroups of a tile's columns hold that tile's jobs under the static deal too), n divides Z, and a tile
has at most 64 jobs.  Auto takes FOUR segments only where all of this holds for four and Z >= 64, else what it takes without
bits.  A launch outside the guard has the plan it has without bits -- same segments, static deal, byte check.

A tile's jobs are jj = sg nxt + xs (sg: z segment, xs: column slot; column xt = (xs + shift sg) % nxt), the static plan's job
number sg ncol + b nxt + xs.  From the bits:
  live        a bit in planes zs - 4 .. zs + LZ + 3, rows x0 - 4 .. x0 + 11 (clipped)            = zwalk_plan_model.live
  rounds_run  rounds (x-rows h .. h + kH - 1, plane z) with a bit within planes z +- 4, rows x0 - 4 + h .. x0 + h + kH + 3
                                                                                                   = zwalk_window_rule
  cost        live ? PLANE_NS * PL + ROUND_NS * rounds_run : FILL_NS
Jobs in the order (cost descending, job number ascending) go one by one to the tile's workgroup with the smallest load,
ties to the lowest.  A workgroup's table is its jobs in that order (the live ones come first by themselves).

  row_bits(occ)                  -> uint32 [B, Z, ceil(X / 32)]
  plan(B, Z, X, Y, segments, bits=True, ...)   -> zwalk_plan_model.plan + "bal"
  deal(rows, p, kH)              -> per workgroup: list of job numbers, and the number of live ones
  cost_us(rows, p, kH)           -> modelled microseconds per workgroup (the plan model's constants)

TRIMMED JOBS (option conv_i8z_trim): after the deal, which does not change, a live job streams only the range from its first
to its last live output plane (live_planes), never fewer than min(8, LZ) outputs; its flanks are filled like dead jobs.
  live_range(rowsb, p, job)      -> (a, len) or None for a dead job
  trimmed_stream(rows, p, kH)    -> per workgroup: [(job number, a, len, S)] and the planes of its stream
  plane_counts(rows, p, kH)      -> (planes streamed, planes trimmed away), as sn_conv_i8z_plane_counts counts them
  cost_us_trimmed(rows, p, kH)   -> cost_us with the trimmed streams
  python tools/debug/zwalk_balanced_model.py   the benchmark's batch: static and balanced plans, max / median / mean"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import zwalk_plan_model as pm  # noqa: E402

PLANE_NS, ROUND_NS, FILL_NS = 520, 122, 300   # kBalPlane, kBalRound, kBalFill
MAX_TILE_JOBS = 64                            # kZBalJobs


def row_bits(occ):
    occ = np.asarray(occ).astype(bool)
    if occ.ndim == 5:
        occ = occ[:, 0]
    B, Z, X, _ = occ.shape
    wx = (X + 31) // 32
    any_y = np.zeros((B, Z, wx * 32), dtype=np.uint64)
    any_y[:, :, :X] = occ.any(axis=-1)
    return (any_y.reshape(B, Z, wx, 32) << np.arange(32, dtype=np.uint64)).sum(axis=-1).astype(np.uint32)


def rows_to_bool(rows, X):
    """[B, Z, wx] uint32 -> [B, Z, X] bool"""
    rows = np.asarray(rows).astype(np.uint32)
    bits = (rows[..., None] >> np.arange(32, dtype=np.uint32)) & 1
    return bits.reshape(rows.shape[0], rows.shape[1], -1)[:, :, :X].astype(bool)


def plan(B, Z, X, Y, segments=0, cus=256, head_only=True, dense=False, bits=True):
    nxt, nyt = (X + pm.K_ZTX - 1) // pm.K_ZTX, (Y + pm.K_TY - 1) // pm.K_TY
    ncol, max_seg = B * nxt * nyt, (Z + 7) // 8

    def bal_ok(m):
        return bool(bits and head_only and not dense and nyt == 1 and Z <= 64 and X <= 64 and ncol == cus
                    and 2 <= m <= max_seg and Z % m == 0 and nxt * m <= MAX_TILE_JOBS)

    seg = segments
    if segments == 0 and Z >= 64 and bal_ok(4) and pm.plan(B, Z, X, Y, 0, cus, head_only, dense)["deal"]:
        seg = 4   # auto: four where the static plan would auto-deal two AND the balanced deal can run; else the no-bits plan
    p = pm.plan(B, Z, X, Y, seg, cus, head_only, dense)
    p["bal"] = int(bool(p["deal"] and p["fill_dead"] and bal_ok(segments if segments >= 2 else p["nseg"])))
    return p


def tile_jobs(p, b):
    """the tile's jobs in job-number order: (job number, (b, x0, y0, zs))"""
    out = []
    for sg in range(p["nseg"]):
        for xs in range(p["nxt"]):
            j = sg * p["ncol"] + b * p["nxt"] + xs
            out.append((j, pm.decode(p, j)[0]))
    return out


def job_cost(rowsb, p, job, kH):
    """(integer cost, live, rounds_run) of one job from the [B, Z, X] row booleans"""
    b, x0, _, zs = job
    Z, X, LZ = p["Z"], p["X"], p["LZ"]
    reg = rowsb[b, max(0, zs - 4):min(Z, zs + LZ + 4), max(0, x0 - 4):min(X, x0 + 12)]
    live = bool(reg.any())
    rounds = 0
    for z in range(zs, min(Z, zs + LZ)):
        win = rowsb[b, max(0, z - 4):min(Z, z + 5)].any(axis=0)
        for h in range(0, min(8, X - x0), kH):
            rounds += int(win[max(0, x0 - 4 + h):min(X, x0 + h + kH + 4)].any())
    return (PLANE_NS * p["PL"] + ROUND_NS * rounds if live else FILL_NS), live, rounds


def deal(rows, p, kH=1):
    """per workgroup: (job numbers in table order, live count).  p must have bal set."""
    assert p["bal"]
    rowsb = rows_to_bool(rows, p["X"])
    nxt = p["nxt"]
    tables = {}
    for b in range(p["B"]):
        jobs = [(j, job) + job_cost(rowsb, p, job, kH) for j, job in tile_jobs(p, b)]
        order = sorted(jobs, key=lambda t: (-t[2], t[0]))
        load = [0] * nxt
        share = [[] for _ in range(nxt)]
        for j, _job, c, lv, _r in order:
            w = min(range(nxt), key=lambda i: (load[i], i))
            load[w] += c
            share[w].append((j, lv))
        for w in range(nxt):
            tables[b * nxt + w] = share[w]
    out = []
    for wg in range(p["grid"]):
        mine = tables[pm.job_id(p, wg, 0)]
        assert all(lv for _, lv in mine[:sum(lv for _, lv in mine)]), "live jobs come first"
        out.append(([j for j, _ in mine], sum(lv for _, lv in mine)))
    return out


def cost_us(rows, p, kH=1):
    """the plan model's microseconds per workgroup, from the bits (static plans: the static tables)"""
    rowsb = rows_to_bool(rows, p["X"])
    if p["bal"]:
        tabs = [[pm.decode(p, j)[0] for j in js] for js, _ in deal(rows, p, kH)]
    else:
        tabs = pm.jobs(p)
    t = []
    for mine in tabs:
        planes = rounds = 0
        for job in mine:
            _, lv, r = job_cost(rowsb, p, job, kH)
            if p["fill_dead"] and not lv:
                continue
            planes += p["PL"]
            rounds += r
        t.append(pm.T_PROLOGUE + pm.T_PLANE * planes + pm.T_ROUND * rounds)
    return np.array(t)


def live_planes(rowsb, p, job):
    """output planes of the job's segment that are LIVE: W[z] -- the OR of the row booleans over planes z - 4 .. z + 4 -- has
    a bit in rows x0 - 4 .. x0 + 11 (clipped).  A plane that is not live has every round empty, for either kH."""
    b, x0, _, zs = job
    Z, X, LZ = p["Z"], p["X"], p["LZ"]
    return [z for z in range(zs, min(Z, zs + LZ))
            if rowsb[b, max(0, z - 4):min(Z, z + 5), max(0, x0 - 4):min(X, x0 + 12)].any()]


def live_range(rowsb, p, job):
    """TRIMMED JOBS (csrc/conv_i8z.inc): (a, len) of a live job -- outputs a .. a + len - 1, from its first to its last live
    plane, at least Lmin = min(8, LZ) of them, extended upwards and moved down where the segment ends first -- or None for a
    dead job (no live plane: the same verdict as job_cost's `live`)."""
    _, _, _, zs = job
    z1 = min(p["Z"], zs + p["LZ"])
    m = live_planes(rowsb, p, job)
    if not m:
        return None
    a, n = m[0], max(m[-1] + 1 - m[0], min(8, p["LZ"]))
    n = min(n, z1 - zs)                 # (a last segment shorter than Lmin: outside the balanced deal's guard)
    if a + n > z1:
        a = z1 - n
    return a, n


def trimmed_stream(rows, p, kH=1, trim=True):
    """per workgroup, under the UNCHANGED deal: [(job number, a, len, S)] of its live jobs in table order -- job k occupies
    stream positions S .. S + len + 8 -- and the planes of its stream.  trim=False: whole segments."""
    rowsb = rows_to_bool(rows, p["X"])
    out = []
    for js, nlive in deal(rows, p, kH):
        S, mine = 0, []
        for j in js[:nlive]:
            job = pm.decode(p, j)[0]
            a, n = live_range(rowsb, p, job) if trim else (job[3], min(p["LZ"], p["Z"] - job[3]))
            mine.append((j, a, n, S))
            S += n + 8
        out.append((mine, S))
    return out


def plane_counts(rows, p, kH=1, trim=True):
    """(planes streamed, planes trimmed away) of one launch: what sn_conv_i8z_plane_counts adds"""
    st = trimmed_stream(rows, p, kH, trim)
    streamed = sum(S for _, S in st)
    return streamed, sum(len(m) for m, _ in st) * p["PL"] - streamed


def cost_us_trimmed(rows, p, kH=1):
    """cost_us with every live job cut to its live range: the same deal, the same rounds run, fewer planes"""
    rowsb = rows_to_bool(rows, p["X"])
    t = []
    for mine, planes in trimmed_stream(rows, p, kH):
        rounds = sum(job_cost(rowsb, p, pm.decode(p, j)[0], kH)[2] for j, _, _, _ in mine)
        t.append(pm.T_PROLOGUE + pm.T_PLANE * planes + pm.T_ROUND * rounds)
    return np.array(t)


def bench_occ():
    root = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.path.insert(0, root)
    from oracle import voxel_oracle as vo
    from scene_net_amd.synthetic import synthetic_tile
    occ = np.zeros((32, 64, 64, 64), dtype=bool)
    for t in range(32):
        c, _, _ = vo.voxel_counts(synthetic_tile(t, 100_000)[0], (64, 64, 64), None, None, None)
        occ[t] = (vo.to_full_dense(vo.normalize_xyz(c.astype(np.float64))) > 0).reshape(64, 64, 64)
    return occ


def main():
    occ = bench_occ()
    rows = row_bits(occ)
    for name, seg, bits in (("2 segments, static shift (no bits)", 2, False), ("4 segments, static shift (no bits)", 4, False),
                            ("2 segments, balanced inside a tile", 2, True), ("4 segments, balanced inside a tile (auto)", 0, True)):
        p = plan(32, 64, 64, 64, seg, bits=bits)
        t = cost_us(rows, p, 1)
        dead = sum(not job_cost(rows_to_bool(rows, 64), p, pm.decode(p, j)[0], 1)[1] for j in range(p["njobs"]))
        print(f"{name}: {p['njobs']} jobs, {dead} dead, bal {p['bal']}; workgroup us max {t.max():.1f} "
              f"median {np.median(t):.1f} mean {t.mean():.1f}")
        if p["bal"]:
            tt = cost_us_trimmed(rows, p, 1)
            print(f"    trimmed to the live ranges, same deal: planes {plane_counts(rows, p, 1, trim=False)[0]} -> "
                  f"{plane_counts(rows, p, 1)[0]}; workgroup us max {tt.max():.1f} median {np.median(tt):.1f} mean {tt.mean():.1f}")


if __name__ == "__main__":
    main()
