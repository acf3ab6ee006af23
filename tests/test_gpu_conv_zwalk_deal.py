"""The z-walk's dealt plan with dead jobs (csrc/conv_i8z.inc "DEAD JOBS", option conv_i8z_segments; the contraction of
SceneNet.forward, core/models/SCENE_Net.py:322-339): a head-only launch cuts its columns into z segments, deals them over the
workgroups, and a workgroup fills the jobs whose operand region holds no set voxel instead of walking them.  Nothing about
the results may show it: every walk call writes into a buffer pre-filled with NaN bits and is compared ON THE RAW BITS with
the same call under conv_i8z_segments = 1 (whole columns, nothing filled) and under conv_i8z_dense = 1, one case per shape
also with sn_conv_bank without a blob (the folded tile kernel); the round counters must be what the numpy rule predicts."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from scene_net_amd import _hip

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", "debug", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


rule = _tool("zwalk_window_rule")
model = _tool("zwalk_plan_model")
KH = {0: 2, 1: 1, 2: 1}                      # x-rows per round of each conv_i8z_variant


def _bank(G, seed):
    g = torch.Generator().manual_seed(seed)
    w = torch.rand((G, 9, 9, 9), generator=g) - 0.5
    w = w + w.flip(2)
    w = w + w.flip(3)
    return (w * torch.logspace(-2, 0.3, G).view(G, 1, 1, 1)).float().contiguous()


def _lam(G, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(G, generator=g) - 0.3) / G


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _walk(x, bank, lam, prep, dt=torch.float32, served=True, out=None):
    """the head-only prepared call into a buffer full of NaN bits -> (out, (rounds run, skipped))"""
    B, _, Z, X, Y = x.shape
    if out is None:
        out = torch.full((B, 1, Z, X, Y), float("nan"), dtype=dt, device=x.device)
    fn = _hip.load().sn_conv_bank_prepared_served if served else _hip.load().sn_conv_bank_prepared
    c0 = _hip.conv_i8z_round_counts()
    rc = fn(x.data_ptr(), _hip.SN_OCC8, bank.data_ptr(), lam.data_ptr(), prep.data_ptr(), B, Z, X, Y, bank.shape[0], 9, 9, 9,
            None, out.data_ptr(), _hip.SN_F32 if dt == torch.float32 else _hip.SN_F64, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    c1 = _hip.conv_i8z_round_counts()
    return out, (c1[0] - c0[0], c1[1] - c0[1])


def _three(occ, bank, lam, prep, seg, dt=torch.float32, variants=(2,), groups=1, tile_kernel=False, served=True):
    """occ (host, bool) under conv_i8z_segments = seg: equal to whole columns and to the dense walk bit for bit, no sentinel
    left, the rule's round counts -> out"""
    x = occ.to(bank.device)
    out = None
    for v in variants:
        want = rule.counts(occ.numpy(), KH[v])
        with _hip.options(conv_i8z_variant=v):
            with _hip.options(conv_i8z_segments=seg):
                out, cnt = _walk(x, bank, lam, prep, dt, served)
            with _hip.options(conv_i8z_segments=1):
                out_p, cnt_p = _walk(x, bank, lam, prep, dt, served)
            with _hip.options(conv_i8z_dense=1):
                out_d, cnt_d = _walk(x, bank, lam, prep, dt, served)
        print(f"variant {v} segments {seg}: rounds {cnt} whole columns {cnt_p} dense {cnt_d} rule {want}")
        assert not bool(torch.isnan(out).any()), (v, "an output was not written")
        assert _same(out, out_p) and _same(out, out_d), v
        assert cnt == cnt_p == (groups * want[0], groups * want[1]), (v, cnt, cnt_p, want)
        assert cnt_d == (groups * (want[0] + want[1]), 0), (v, cnt_d)
    if tile_kernel:
        assert _same(out, _hip.conv_bank(x, bank, lam, out_dtype=dt)[1])
    assert _hip.device_status()[0] == 0
    return out


def _dead(occ, seg):
    """(dead jobs, jobs) of the plan the launch takes"""
    B, _, Z, X, Y = occ.shape
    p = model.plan(B, Z, X, Y, seg, cus=torch.cuda.get_device_properties(0).multi_processor_count)
    assert p["fill_dead"] == 1, p
    o = occ[:, 0].numpy()
    return sum(not model.live(o, p, j) for mine in model.jobs(p) for j in mine), p["njobs"]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def bank16(dev):
    bank, lam = _bank(16, 3).to(dev), _lam(16, 4).to(dev)
    prep = _hip.conv_bank_prep(bank)
    _hip.conv_bank(torch.zeros((1, 1, 16, 8, 16), dtype=torch.bool, device=dev), bank, lam, prep=prep)   # (the verdict: served)
    return bank, lam, prep


# (B, Z, X, Y, segments): a ring-sized stream per job (Z = 16: LZ = 8), a last segment shorter (Z = 33), Z = 32; X = 9 and 16
# (two columns in x), X = 24 (three: the shift is not half); Y = 16, 64, 80 (two y tiles)
SHAPES = [(2, 16, 16, 64, 2), (3, 33, 16, 64, 2), (2, 32, 9, 64, 2), (2, 32, 24, 64, 2), (5, 32, 16, 16, 2), (1, 32, 16, 80, 2)]


@pytest.mark.parametrize("B,Z,X,Y,seg", SHAPES)
def test_all_zero_every_job_is_dead(dev, bank16, B, Z, X, Y, seg):
    """no workgroup walks: every output is the fill's + 0.0"""
    bank, lam, prep = bank16
    occ = torch.zeros((B, 1, Z, X, Y), dtype=torch.bool)
    dead, n = _dead(occ, seg)
    assert dead == n
    out = _three(occ, bank, lam, prep, seg, variants=(0, 1, 2), tile_kernel=True)
    assert bool((_bits(out) == 0).all())
    _three(occ, bank, lam, prep, seg, served=False)


@pytest.mark.parametrize("B,Z,X,Y,seg", SHAPES)
def test_halves(dev, bank16, B, Z, X, Y, seg):
    """the lower half in z empty and the upper random 30 %, and the reverse: the jobs of one half are dead"""
    bank, lam, prep = bank16
    g = torch.Generator().manual_seed(Z * 1000 + X * 10 + Y)
    for upper in (True, False):
        occ = torch.zeros((B, 1, Z, X, Y), dtype=torch.bool)
        half = torch.rand((B, 1, Z // 2 - 4, X, Y), generator=g) < 0.3
        if upper:
            occ[:, :, Z - half.shape[2]:] = half
        else:
            occ[:, :, :half.shape[2]] = half
        dead, n = _dead(occ, seg)
        assert 0 < dead < n, (dead, n)
        _three(occ, bank, lam, prep, seg, variants=(0, 1, 2) if upper else (2,), tile_kernel=upper)


def test_one_voxel_at_each_face_of_a_jobs_region_and_one_step_outside(dev, bank16):
    """Z = 32 in two segments, X = 24, Y = 80: the job (x0 = 8, y0 = 0, zs = 0) for the upper z face, (8, 0, 16) for the lower,
    (8, 64, 0) for the low y face; a voxel ON a face makes the job live, one step outside leaves it dead -- and the results
    and counters are the rule's either way.  Then the grid's corners (clipped regions)."""
    bank, lam, prep = bank16
    B, Z, X, Y, seg = 1, 32, 24, 80, 2
    p = model.plan(B, Z, X, Y, seg, cus=torch.cuda.get_device_properties(0).multi_processor_count)
    assert p["LZ"] == 16
    lo, up, y1 = (0, 8, 0, 16), (0, 8, 0, 0), (0, 8, 64, 0)
    cases = [(lo, (12, 10, 30), True), (lo, (11, 10, 30), False),          # planes zs - 4 / zs - 5
             (up, (19, 10, 30), True), (up, (20, 10, 30), False),          # planes zs + LZ + 3 / zs + LZ + 4
             (up, (5, 4, 30), True), (up, (5, 3, 30), False),              # rows x0 - 4 / x0 - 5
             (up, (5, 19, 30), True), (up, (5, 20, 30), False),            # rows x0 + 11 / x0 + 12
             (y1, (5, 10, 60), True), (y1, (5, 10, 59), False),            # y0 - 4 / y0 - 5
             (up, (5, 10, 67), True), (up, (5, 10, 68), False),            # y0 + 67 / y0 + 68
             ((0, 0, 0, 0), (0, 0, 0), True), (lo, (31, 23, 79), False), ((0, 16, 64, 16), (31, 23, 79), True)]
    for i, (job, (z, xx, y), is_live) in enumerate(cases):
        occ = torch.zeros((B, 1, Z, X, Y), dtype=torch.bool)
        occ[0, 0, z, xx, y] = True
        assert model.live(occ[:, 0].numpy(), p, job) == is_live, (job, z, xx, y)
        out = _three(occ, bank, lam, prep, seg, variants=(0, 1, 2) if i in (0, 5, 12) else (2,), tile_kernel=i in (0, 1))
        assert bool((out != 0).any())


def test_random_half_occupancy_nothing_is_dead(dev, bank16):
    bank, lam, prep = bank16
    g = torch.Generator().manual_seed(50)
    occ = torch.rand((2, 1, 32, 16, 64), generator=g) < 0.5
    assert _dead(occ, 2)[0] == 0
    _three(occ, bank, lam, prep, 2, variants=(0, 1, 2), tile_kernel=True)


def test_300_columns_in_two_segments_several_jobs_per_workgroup(dev, bank16):
    """B = 150, X = 16: 300 columns x 2 segments on the chip's workgroups -- two or three jobs each, dead ones between live
    ones (every third tile carries voxels, in one half of z and one column)"""
    bank, lam, prep = bank16
    occ = torch.zeros((150, 1, 16, 16, 16), dtype=torch.bool)
    g = torch.Generator().manual_seed(300)
    for b in range(0, 150, 3):
        z0, x0 = (0, 0) if b % 2 == 0 else (13, 13)
        occ[b, 0, z0:z0 + 3, x0:x0 + 3] = torch.rand((3, 3, 16), generator=g) < 0.4
    dead, n = _dead(occ, 2)
    assert n == 600 and 300 < dead < 600
    _three(occ, bank, lam, prep, 2, variants=(0, 1, 2), tile_kernel=True)


@pytest.mark.parametrize("dt", [torch.float32, torch.float64], ids=["fp32", "fp64"])
def test_two_groups_accumulate_into_one_head(dev, dt):
    """G = 20: the second group's launch loads what the first stored, adds and activates (head & 1) -- in its filled jobs too"""
    bank, lam = _bank(20, 7).to(dev), _lam(20, 8).to(dev)
    prep = _hip.conv_bank_prep(bank)
    g = torch.Generator().manual_seed(20)
    occ = torch.zeros((2, 1, 32, 16, 48), dtype=torch.bool)
    occ[:, :, 20:] = torch.rand((2, 1, 12, 16, 48), generator=g) < 0.2
    _hip.conv_bank(occ.to(dev), bank, lam, prep=prep)
    assert _dead(occ, 2)[0] > 0
    _three(occ, bank, lam, prep, 2, dt=dt, variants=(0, 2), groups=2, tile_kernel=True)
    out = _three(torch.zeros_like(occ), bank, lam, prep, 2, dt=dt, groups=2)
    assert bool((_bits(out) == 0).all())


@pytest.mark.parametrize("where", ["head", "bank"])
def test_a_nan_coefficient_fills_nothing(dev, bank16, where):
    """head: a NaN among the head's coefficients reaches the walk (test_gpu_conv_zwalk_skip.py) and switches the skip off --
    no job is dead, nothing is filled, every round runs and NaN x 0 = NaN propagates, exactly as with whole columns.
    bank: a NaN tap (the centre: the bank stays symmetric) does not survive the 24-bit quantisation, with either plan: the
    launch skips, and the dealt plan's results and counters are the parent plan's."""
    bank, lam, _ = bank16
    bank, lam = bank.clone(), lam.clone()
    if where == "head":
        lam[5] = float("nan")
    else:
        bank[5, 4, 4, 4] = float("nan")
    prep = _hip.conv_bank_prep(bank)
    occ = torch.zeros((2, 1, 32, 16, 64), dtype=torch.bool)
    occ[0, 0, 3, 3, 3] = True
    assert _dead(occ, 2)[0] == 7
    x = occ.to(dev)
    with _hip.options(conv_i8z_segments=2):
        out, cnt = _walk(x, bank, lam, prep, served=False)
    with _hip.options(conv_i8z_segments=1):
        out_p, cnt_p = _walk(x, bank, lam, prep, served=False)
    print(where, "nan: rounds", cnt, cnt_p, "nan outputs", int(torch.isnan(out).sum()), "of", out.numel())
    assert _same(out, out_p) and cnt == cnt_p
    if where == "head":
        assert cnt == (sum(rule.counts(occ.numpy(), 1)), 0)
        assert bool(torch.isnan(out).all())
    assert _hip.device_status()[0] == 0


@pytest.mark.parametrize("seg", [3, 4])
def test_three_and_four_segments(dev, bank16, seg):
    bank, lam, prep = bank16
    g = torch.Generator().manual_seed(seg)
    occ = torch.zeros((2, 1, 32, 16, 64), dtype=torch.bool)
    occ[:, :, :6] = torch.rand((2, 1, 6, 16, 64), generator=g) < 0.1
    dead, n = _dead(occ, seg)
    assert n == 2 * 2 * seg and 0 < dead < n
    _three(occ, bank, lam, prep, seg, variants=(0, 1, 2), tile_kernel=True)


def test_auto_deals_a_launch_of_whole_columns(dev, bank16):
    """B = 128, X = 16, Y = 16, Z = 32: 256 columns, which the dense plan walks whole -- the default (0) takes two segments"""
    bank, lam, prep = bank16
    g = torch.Generator().manual_seed(128)
    occ = torch.zeros((128, 1, 32, 16, 16), dtype=torch.bool)
    occ[::2, :, :5, :8] = torch.rand((64, 1, 5, 8, 16), generator=g) < 0.1
    dead, n = _dead(occ, 0)
    assert n == 512 and dead >= 256
    assert _hip.get_option("conv_i8z_segments") == 0
    _three(occ, bank, lam, prep, 0, variants=(0, 1, 2), tile_kernel=True)


def test_a_captured_call_with_dead_jobs_replays(dev, bank16):
    bank, lam, prep = bank16
    g = torch.Generator().manual_seed(9)
    occ = torch.zeros((2, 1, 32, 16, 64), dtype=torch.bool)
    occ[:, :, 22:] = torch.rand((2, 1, 10, 16, 64), generator=g) < 0.2
    assert _dead(occ, 2)[0] > 0
    x = occ.to(dev)
    with _hip.options(conv_i8z_segments=2):
        eager, _ = _walk(x, bank, lam, prep)
        got = torch.full_like(eager, float("nan"))
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            with torch.cuda.graph(graph, stream=side):
                rc = _hip.load().sn_conv_bank_prepared_served(
                    x.data_ptr(), _hip.SN_OCC8, bank.data_ptr(), lam.data_ptr(), prep.data_ptr(), 2, 32, 16, 64, 16, 9, 9, 9,
                    None, got.data_ptr(), _hip.SN_F32, torch.cuda.current_stream().cuda_stream)
                assert rc == 0
        torch.cuda.current_stream().wait_stream(side)
    for _ in range(2):
        got.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert _same(got, eager)
    assert _hip.device_status()[0] == 0
