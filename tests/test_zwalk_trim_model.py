"""The z-walk's trimmed jobs (csrc/conv_i8z.inc "TRIMMED JOBS", option conv_i8z_trim) on the host (no GPU): the live-range
rule of tools/debug/zwalk_balanced_model.py against the window rule computed from the occupancy bytes, its padding, what a
superset of the bits does, the model's figures for the benchmark's batch, the hand-over protocol on streams of jobs of
different lengths (tools/debug/zwalk_protocol_sim.py), and the option and the counter in the header, the table and the
binding."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest

from scene_net_amd import _hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", "debug", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


bal = _tool("zwalk_balanced_model")
sim = _tool("zwalk_protocol_sim")
SHAPES = [(32, 64, 64, 16), (64, 64, 32, 16), (32, 32, 64, 16)]   # under the balanced deal's guard with 256 compute units


def _jobs(p):
    return [bal.pm.decode(p, j)[0] for j in range(p["njobs"])]


def _hand_made(B, Z, X, Y, seed):
    """a few tiles: sparse noise in a slab, a full-height column, single voxels next to segment boundaries and grid faces"""
    rng = np.random.default_rng(seed)
    occ = np.zeros((B, Z, X, Y), dtype=bool)
    occ[0, 3:9] = rng.random((6, X, Y)) < 0.002
    occ[1, :, 5, 3] = True
    occ[2, Z // 2 - 5, X - 1, 0] = True
    occ[2, Z // 2 + 3, 0, Y - 1] = True
    occ[3, 0, 12, 5] = True
    occ[3, Z - 1, 13, 5] = True
    occ[4, 1, 20, 3] = True
    occ[4, 14, 20, 3] = True
    occ[5] = rng.random((Z, X, Y)) < 0.0005
    return occ


@pytest.mark.parametrize("B,Z,X,Y", SHAPES)
def test_the_live_range_is_the_window_rule_of_the_bytes(B, Z, X, Y):
    occ = _hand_made(B, Z, X, Y, Z + X)
    p = bal.plan(B, Z, X, Y, 0)
    assert p["bal"] == 1
    rowsb = bal.rows_to_bool(bal.row_bits(occ), X)
    lmin = min(8, p["LZ"])
    trimmed = 0
    for job in _jobs(p):
        b, x0, _, zs = job
        z1 = min(Z, zs + p["LZ"])
        live = [z for z in range(zs, z1) if occ[b, max(0, z - 4):z + 5, max(0, x0 - 4):x0 + 12].any()]
        assert bal.live_planes(rowsb, p, job) == live
        r = bal.live_range(rowsb, p, job)
        # dead == no live plane == the deal's own verdict
        assert (r is None) == (not live) == (not bal.job_cost(rowsb, p, job, 1)[1])
        if r is None:
            continue
        a, n = r
        assert zs <= a and a + n <= z1 and n >= lmin and a <= live[0] and live[-1] < a + n
        assert n == max(live[-1] + 1 - live[0], lmin), "no longer than the rule asks"
        trimmed += z1 - zs - n
        for z in list(range(zs, a)) + list(range(a + n, z1)):
            for kH in (1, 2):
                for h in range(0, min(8, X - x0), kH):
                    assert not occ[b, max(0, z - 4):z + 5, max(0, x0 - 4 + h):x0 + h + kH + 4].any(), (job, z, kH, h)
    assert trimmed > 0


def test_ranges_are_padded_inside_the_segment_at_both_ends():
    """(32, 32, 64, 16): two segments of 16 planes, one voxel"""
    B, Z, X, Y = SHAPES[2]
    p = bal.plan(B, Z, X, Y, 0)
    assert p["bal"] == 1 and p["LZ"] == 16
    want = {11: [(7, 9)], 12: [(8, 8), (16, 8)], 19: [(8, 8), (16, 8)], 20: [(16, 9)], 31: [(24, 8)], 0: [(0, 8)],
            15: [(8, 8), (16, 8)], 16: [(8, 8), (16, 8)]}
    for z, ranges in want.items():
        occ = np.zeros((B, Z, X, Y), dtype=bool)
        occ[3, z, 30, 7] = True
        rowsb = bal.rows_to_bool(bal.row_bits(occ), X)
        got = sorted({r for r in (bal.live_range(rowsb, p, job) for job in _jobs(p)) if r is not None})
        assert got == ranges, (z, got)
    # a short last segment is never longer than itself (outside the balanced deal's guard, for the rule's sake)
    q = dict(p, Z=28)
    occ = np.zeros((B, 28, X, Y), dtype=bool)
    occ[3, 27, 30, 7] = True
    got = {bal.live_range(bal.rows_to_bool(bal.row_bits(occ), X), q, job) for job in _jobs(p)} - {None}
    assert got == {(20, 8)}


def test_a_superset_of_the_bits_gives_ranges_that_contain_the_true_ones():
    B, Z, X, Y = SHAPES[0]
    occ = _hand_made(B, Z, X, Y, 7)
    p = bal.plan(B, Z, X, Y, 0)
    rows = bal.row_bits(occ)
    rng = np.random.default_rng(1)
    extra = rng.integers(0, 2 ** 32, size=rows.shape, dtype=np.uint64).astype(np.uint32)
    for _ in range(6):
        extra &= rng.integers(0, 2 ** 32, size=rows.shape, dtype=np.uint64).astype(np.uint32)
    true_b, more_b = bal.rows_to_bool(rows, X), bal.rows_to_bool(rows | extra, X)
    grew = 0
    for job in _jobs(p):
        t, m = bal.live_range(true_b, p, job), bal.live_range(more_b, p, job)
        if t is None:
            continue
        assert m is not None and m[0] <= t[0] and t[0] + t[1] <= m[0] + m[1], (job, t, m)
        grew += m[1] - t[1]
    assert grew > 0
    assert bal.plane_counts(rows | extra, p)[0] > bal.plane_counts(rows, p)[0]


def test_the_stream_follows_the_unchanged_deal():
    B, Z, X, Y = SHAPES[1]
    occ = _hand_made(B, Z, X, Y, 3)
    p = bal.plan(B, Z, X, Y, 0)
    rows = bal.row_bits(occ)
    tables, streams, whole = bal.deal(rows, p, 1), bal.trimmed_stream(rows, p, 1), bal.trimmed_stream(rows, p, 1, trim=False)
    for (ids, nlive), (mine, planes), (mine_w, planes_w) in zip(tables, streams, whole):
        assert [j for j, _, _, _ in mine] == ids[:nlive] == [j for j, _, _, _ in mine_w]
        at = 0
        for _, _, n, S in mine:
            assert S == at
            at += n + 8
        assert planes == at and planes_w == nlive * p["PL"]
    assert bal.plane_counts(rows, p, 1, trim=False) == (sum(n for _, n in tables) * p["PL"], 0)
    s, t = bal.plane_counts(rows, p, 1)
    assert t > 0 and s + t == sum(n for _, n in tables) * p["PL"]


def test_the_benchmarks_batch():
    """32 synthetic tiles of 100 k points at 64^3, four segments dealt by cost: the figures DESIGN section 4 quotes"""
    rows = bal.row_bits(bal.bench_occ())
    p = bal.plan(32, 64, 64, 64, 0)
    assert p["bal"] == 1 and p["nseg"] == 4
    assert bal.plane_counts(rows, p, 1, trim=False) == (11664, 0)
    assert bal.plane_counts(rows, p, 1) == (10085, 11664 - 10085)
    before, after = bal.cost_us(rows, p, 1), bal.cost_us_trimmed(rows, p, 1)
    assert (round(before.max(), 1), round(after.max(), 1)) == (57.8, 50.2)
    assert (round(float(np.median(before)), 1), round(float(np.median(after)), 1)) == (44.9, 40.7)
    assert (round(before.mean(), 1), round(after.mean(), 1)) == (44.5, 41.3)


@pytest.mark.parametrize("kTPS,nwaves", [(4, 12), (8, 12), (8, 8)])     # the three shapes sn_set_option("conv_i8z_variant") offers
@pytest.mark.parametrize("lens", sim.MIXED, ids=lambda v: "-".join(map(str, v)))
def test_the_protocol_has_no_hazard_on_mixed_length_streams(kTPS, nwaves, lens):
    for skip in (0.0, 0.3):
        for adversarial in (False, True):
            for seed in range(3):
                assert sim.simulate(0, 0, kTPS, nwaves, seed, ordered_reads=True, skip_prob=skip, adversarial=adversarial,
                                    lens=lens)


@pytest.mark.parametrize("kTPS,nwaves", [(4, 12), (8, 12)])
def test_a_round_frozen_at_a_short_jobs_end_finds_nothing(kTPS, nwaves):
    """the directed adversary at every slot around the seams of 16-plane jobs and at the stream's end"""
    lens = [8, 16, 8, 8]
    NPL = sum(n + 8 for n in lens)
    for fs in range(0, NPL + 3):
        assert sim.simulate(0, 0, kTPS, nwaves, fs & 1, ordered_reads=True, adversarial=False, freeze_slot=fs, lens=lens)


def test_uniform_lens_are_the_uniform_stream():
    for seed in range(3):
        assert sim.simulate(3, 8, 4, 12, seed) and sim.simulate(0, 0, 4, 12, seed, lens=[8, 8, 8])


# ------------------------------------------------------------------------------------------ the option and the counter
def test_the_option_is_documented_and_in_the_table():
    header = open(os.path.join(ROOT, "include", "scenenet_hip.h")).read()
    assert '"conv_i8z_trim" (switch, default 1)' in header
    table = open(os.path.join(ROOT, "scene-net_amd", "csrc", "cabi.hip")).read()
    enum = open(os.path.join(ROOT, "scene-net_amd", "csrc", "common.h")).read()
    assert re.search(r'\{"conv_i8z_trim",\s+nullptr,\s+0,\s+1,\s+0,\s+1,\s+true\}', table)
    names = re.findall(r'^\s+\{"(\w+)",', table, flags=re.M)
    kopts = re.findall(r"^\s+kOpt(\w+),", enum, flags=re.M)
    assert len(names) == len(kopts) and names.index("conv_i8z_trim") == kopts.index("ConvI8zTrim")


def test_the_option_round_trips_and_defaults_to_one():
    assert _hip.get_option("conv_i8z_trim") == 1
    with _hip.options(conv_i8z_trim=0):
        assert _hip.get_option("conv_i8z_trim") == 0
        with _hip.options(conv_i8z_trim=7):
            assert _hip.get_option("conv_i8z_trim") == 1
    assert _hip.get_option("conv_i8z_trim") == 1


def test_plane_counts_symbol_is_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "scenenet_hip.h")).read()
    assert re.search(r"int sn_conv_i8z_plane_counts\(unsigned long long\* counts2\);", header)
    assert "sn_conv_i8z_plane_counts" in _hip.SYMBOLS and callable(_hip.conv_i8z_plane_counts)
    lib = ctypes.CDLL(_hip.LIB_PATH)
    lib.sn_conv_i8z_plane_counts.argtypes = [ctypes.c_void_p]
    assert lib.sn_conv_i8z_plane_counts(None) == -1
