"""The z-walk's trimmed jobs (csrc/conv_i8z.inc "TRIMMED JOBS", option conv_i8z_trim): where the balanced deal stands a live
job streams only the range from its first to its last live output plane, at least min(8, LZ) planes, and its flanks are
filled in the prologue.  Nothing about the results may show it: every call writes into a buffer pre-filled with NaN bits and is
compared ON THE RAW BITS with the same call under conv_i8z_trim = 0, with the call without bits under conv_i8z_segments = 1
(whole columns) and with the call under conv_i8z_dense = 1.  The round counters must be what the numpy rule predicts, the
plane counters (sn_conv_i8z_plane_counts) what the model predicts (tools/debug/zwalk_balanced_model.py: trimmed_stream), the
device status 0 and no spin may have given up."""
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
bal = _tool("zwalk_balanced_model")
KH = {0: 2, 1: 1, 2: 1}                      # x-rows per round of each conv_i8z_variant
SHAPES = [(32, 64, 64, 16), (64, 64, 32, 16), (32, 32, 64, 16)]   # (B, Z, X, Y): 256 columns; four, four, two segments
OFF = (16, 64, 64, 16)                       # 128 columns: off the guard, the static deal of two segments


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


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _walk(x, bank, lam, prep, rows=None, dt=torch.float32, served=True):
    """the head-only prepared call into a buffer full of NaN bits -> (out, (rounds run, skipped), (planes streamed, trimmed))"""
    B, _, Z, X, Y = x.shape
    out = torch.full((B, 1, Z, X, Y), float("nan"), dtype=dt, device=x.device)
    c0, p0 = _hip.conv_i8z_round_counts(), _hip.conv_i8z_plane_counts()
    rc = _hip.load().sn_conv_bank_prepared_rows(
        x.data_ptr(), _hip.SN_OCC8, bank.data_ptr(), lam.data_ptr(), prep.data_ptr(), B, Z, X, Y, bank.shape[0], 9, 9, 9,
        None, out.data_ptr(), _hip.SN_F32 if dt == torch.float32 else _hip.SN_F64, torch.cuda.current_stream().cuda_stream,
        int(served), None if rows is None else rows.data_ptr(), None)
    assert rc == 0, rc
    c1, p1 = _hip.conv_i8z_round_counts(), _hip.conv_i8z_plane_counts()
    return out, (c1[0] - c0[0], c1[1] - c0[1]), (p1[0] - p0[0], p1[1] - p0[1])


def _check(occ, bank, lam, prep, rows=None, dt=torch.float32, variants=(2,), groups=1):
    """occ (host, bool) with bits (the true ones unless `rows`, a host uint32 array, is given) -> (out, planes, streams)"""
    dev = bank.device
    x = occ.to(dev)
    B, _, Z, X, Y = occ.shape
    rows_h = bal.row_bits(occ.numpy()) if rows is None else rows
    rows_d = torch.from_numpy(rows_h.view(np.int32)).to(dev)
    p = bal.plan(B, Z, X, Y, 0, cus=_cus())
    spins = _hip.conv_i8_spin_timeouts()
    out = planes = streams = None
    for v in variants:
        want = rule.counts(occ.numpy(), KH[v])
        with _hip.options(conv_i8z_variant=v):
            assert _hip.get_option("conv_i8z_trim") == 1
            out, cnt, planes = _walk(x, bank, lam, prep, rows_d, dt)
            with _hip.options(conv_i8z_trim=0):
                out_0, cnt_0, planes_0 = _walk(x, bank, lam, prep, rows_d, dt)
            with _hip.options(conv_i8z_segments=1):
                out_p, cnt_p, _ = _walk(x, bank, lam, prep, None, dt)
            with _hip.options(conv_i8z_dense=1):
                out_d, cnt_d, planes_d = _walk(x, bank, lam, prep, rows_d, dt)
        print(f"variant {v}: bal {p['bal']} rounds {cnt} planes {planes} untrimmed {planes_0} dense {planes_d} rule {want}")
        assert not bool(torch.isnan(out).any()), (v, "an output was not written")
        assert _same(out, out_0) and _same(out, out_p) and _same(out, out_d), v
        assert cnt == cnt_0 == cnt_p == (groups * want[0], groups * want[1]), (v, cnt, cnt_0, cnt_p, want)
        assert cnt_d == (groups * (want[0] + want[1]), 0), (v, cnt_d)
        assert planes_0[1] == 0 and planes_d[1] == 0 and planes[0] + planes[1] == planes_0[0], (v, planes, planes_0, planes_d)
        if p["bal"]:
            streams = bal.trimmed_stream(rows_h, p, KH[v])
            streamed = sum(S for _, S in streams)
            whole = sum(len(m) for m, _ in streams) * p["PL"]
            assert planes == (groups * streamed, groups * (whole - streamed)), (v, planes, streamed, whole)
            assert planes_0 == (groups * whole, 0), (v, planes_0, whole)
        else:
            assert planes[1] == 0, "off the guard nothing is trimmed"
    assert _hip.device_status()[0] == 0 and _hip.conv_i8_spin_timeouts() == spins
    return out, planes, streams


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


def _ground_and_towers(B, Z, X, Y, seed):
    """ground in z <= 12 everywhere (5 %), two columns of full height in two tiles"""
    g = torch.Generator().manual_seed(seed)
    occ = torch.zeros((B, 1, Z, X, Y), dtype=torch.bool)
    occ[:, :, :13] = torch.rand((B, 1, 13, X, Y), generator=g) < 0.05
    occ[1, 0, :, 3:5, 4:9] = True
    occ[1, 0, :, X - 6:X - 3, 2:6] = True
    occ[B - 2, 0, :, 10:12, 8:12] = True
    occ[B - 2, 0, :, 17:19, 1:3] = True
    return occ


@pytest.mark.parametrize("B,Z,X,Y", SHAPES + [OFF])
def test_ground_and_two_towers(dev, bank16, B, Z, X, Y):
    bank, lam, prep = bank16
    occ = _ground_and_towers(B, Z, X, Y, Z + X)
    assert bal.plan(B, Z, X, Y, 0, cus=_cus())["bal"] == int((B, Z, X, Y) != OFF)
    out, planes, _ = _check(occ, bank, lam, prep, variants=(0, 1, 2) if (B, Z, X, Y) == SHAPES[0] else (2,))
    assert bool((out != 0).any())
    if (B, Z, X, Y) != OFF:
        assert planes[1] > 0, "ground in z <= 12: the segment above it is live in its first plane only"


@pytest.mark.parametrize("z", [11, 12, 19, 20, 31, 0])
def test_a_single_voxel(dev, bank16, z):
    """(32, 32, 64, 16): two segments of 16 planes.  z = 12 makes plane 16 the upper segment's only live plane, z = 19 makes
    plane 15 the lower one's: ranges of one plane on either side of the boundary, padded to eight (upwards; downwards where
    the segment ends first).  z = 11 and z = 20 stay inside one segment; z = 0 and z = Z - 1 sit at the grid's ends."""
    bank, lam, prep = bank16
    B, Z, X, Y = SHAPES[2]
    occ = torch.zeros((B, 1, Z, X, Y), dtype=torch.bool)
    occ[3, 0, z, 30, 7] = True
    out, planes, streams = _check(occ, bank, lam, prep)
    assert bool((out != 0).any())
    ranges = sorted({(a, n) for mine, _ in streams for _, a, n, _ in mine})
    want = {11: [(7, 9)], 12: [(8, 8), (16, 8)], 19: [(8, 8), (16, 8)], 20: [(16, 9)], 31: [(24, 8)], 0: [(0, 8)]}[z]
    assert ranges == want, (z, ranges)
    assert planes[1] > 0


def test_two_live_runs_with_an_empty_gap_stay_one_range(dev, bank16):
    """a voxel at z = 1 and one at z = 14 of the same column: planes 0 .. 5 and 10 .. 15 are live, 6 .. 9 are not -- interior
    empty planes are streamed (out of scope), the range is the whole segment"""
    bank, lam, prep = bank16
    B, Z, X, Y = SHAPES[0]
    occ = torch.zeros((B, 1, Z, X, Y), dtype=torch.bool)
    occ[5, 0, 1, 20, 3] = True
    occ[5, 0, 14, 20, 3] = True
    _, planes, streams = _check(occ, bank, lam, prep)
    ranges = sorted({(a, n) for mine, _ in streams for _, a, n, _ in mine})
    assert ranges == [(0, 16), (16, 8)], ranges


def test_random_half_occupancy_trims_nothing(dev, bank16):
    bank, lam, prep = bank16
    B, Z, X, Y = SHAPES[1]
    g = torch.Generator().manual_seed(50)
    occ = torch.rand((B, 1, Z, X, Y), generator=g) < 0.5
    _, planes, _ = _check(occ, bank, lam, prep)
    assert planes == (B * ((X + 7) // 8) * 4 * 24, 0)


@pytest.mark.parametrize("B,Z,X,Y", [SHAPES[0], SHAPES[2], OFF])
def test_all_zero(dev, bank16, B, Z, X, Y):
    bank, lam, prep = bank16
    out, planes, _ = _check(torch.zeros((B, 1, Z, X, Y), dtype=torch.bool), bank, lam, prep)
    assert bool((_bits(out) == 0).all())
    # (off the guard this shape has the dense walk's plan, two static segments per column: everything is streamed)
    assert planes == ((0, 0) if (B, Z, X, Y) != OFF else (B * ((X + 7) // 8) * 2 * 40, 0))


def test_a_superset_of_the_bits_gives_the_same_output_and_more_planes(dev, bank16):
    bank, lam, prep = bank16
    B, Z, X, Y = SHAPES[0]
    occ = _ground_and_towers(B, Z, X, Y, 77)
    true_rows = bal.row_bits(occ.numpy())
    ref, planes, _ = _check(occ, bank, lam, prep)
    rng = np.random.default_rng(5)
    extra = rng.integers(0, 2 ** 32, size=true_rows.shape, dtype=np.uint64).astype(np.uint32)
    for _ in range(4):                          # (about 6 % of the rows)
        extra &= rng.integers(0, 2 ** 32, size=true_rows.shape, dtype=np.uint64).astype(np.uint32)
    out, more, _ = _check(occ, bank, lam, prep, rows=true_rows | extra)
    assert _same(out, ref) and more[0] > planes[0]
    out, full, _ = _check(occ, bank, lam, prep, rows=np.full_like(true_rows, 0xffffffff))
    assert _same(out, ref) and full == (B * ((X + 7) // 8) * 4 * 24, 0)


def test_fp64_head(dev, bank16):
    bank, lam, prep = bank16
    _, planes, _ = _check(_ground_and_towers(*SHAPES[1], 64), bank, lam, prep, dt=torch.float64, variants=(0, 2))
    assert planes[1] > 0


@pytest.mark.parametrize("dt", [torch.float32, torch.float64], ids=["fp32", "fp64"])
def test_two_groups_accumulate_into_one_head(dev, dt):
    """G = 20: the second group's launch loads what the first stored, adds and activates (head & 1) -- in the flanks too"""
    bank, lam = _bank(20, 7).to(dev), _lam(20, 8).to(dev)
    prep = _hip.conv_bank_prep(bank)
    occ = _ground_and_towers(*SHAPES[1], 20)
    _hip.conv_bank(occ.to(dev), bank, lam, prep=prep)
    _, planes, _ = _check(occ, bank, lam, prep, dt=dt, groups=2)
    assert planes[1] > 0


def test_a_nan_coefficient_trims_nothing(dev, bank16):
    bank, lam, _ = bank16
    bank, lam = bank.clone(), lam.clone()
    lam[5] = float("nan")
    prep = _hip.conv_bank_prep(bank)
    B, Z, X, Y = SHAPES[1]
    occ = _ground_and_towers(B, Z, X, Y, 9)
    x = occ.to(dev)
    rows = _hip.row_bits_of(x)
    spins = _hip.conv_i8_spin_timeouts()
    out, cnt, planes = _walk(x, bank, lam, prep, rows, served=False)
    with _hip.options(conv_i8z_segments=1):
        out_p, cnt_p, _ = _walk(x, bank, lam, prep, None, served=False)
    assert _same(out, out_p) and cnt == cnt_p == (sum(rule.counts(occ.numpy(), 1)), 0)
    assert bool(torch.isnan(out).all())
    assert planes == (B * ((X + 7) // 8) * 4 * 24, 0), "the static deal: every job whole"
    assert _hip.device_status()[0] == 0 and _hip.conv_i8_spin_timeouts() == spins


def test_a_captured_call_replays_on_refilled_input(dev, bank16):
    bank, lam, prep = bank16
    B, Z, X, Y = SHAPES[1]
    first, second = _ground_and_towers(B, Z, X, Y, 11), _ground_and_towers(B, Z, X, Y, 12).flip(2)
    second[:B // 2] = False                    # (half the tiles empty: other rounds, other planes than `first`)
    x = first.to(dev)
    got = torch.full((B, 1, Z, X, Y), float("nan"), device=dev)
    p = bal.plan(B, Z, X, Y, 0, cus=_cus())
    assert p["bal"] == 1
    # what the rule and the model say of each input: rounds (run, skipped), planes (streamed, trimmed away)
    want = {}
    for name, occ in (("first", first), ("second", second)):
        streams = bal.trimmed_stream(bal.row_bits(occ.numpy()), p, 1)
        streamed = sum(S for _, S in streams)
        want[name] = (rule.counts(occ.numpy(), 1), (streamed, sum(len(m) for m, _ in streams) * p["PL"] - streamed))
    assert want["first"][1] != want["second"][1] and want["first"][1][1] > 0 and want["second"][1][1] > 0
    spins = _hip.conv_i8_spin_timeouts()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            rows = _hip.row_bits_of(x)          # (made inside the capture: torch's allocator, no sync)
            rc = _hip.load().sn_conv_bank_prepared_rows(
                x.data_ptr(), _hip.SN_OCC8, bank.data_ptr(), lam.data_ptr(), prep.data_ptr(), B, Z, X, Y, 16, 9, 9, 9,
                None, got.data_ptr(), _hip.SN_F32, torch.cuda.current_stream().cuda_stream, 1, rows.data_ptr(), None)
            assert rc == 0
    torch.cuda.current_stream().wait_stream(side)
    for name, occ in (("first", first), ("second", second), ("first", first)):
        x.copy_(occ.to(dev))
        with _hip.options(conv_i8z_trim=0):
            eager, _, _ = _walk(x, bank, lam, prep, _hip.row_bits_of(x))
        got.fill_(float("nan"))
        c0, p0 = _hip.conv_i8z_round_counts(), _hip.conv_i8z_plane_counts()
        graph.replay()
        torch.cuda.synchronize()
        c1, p1 = _hip.conv_i8z_round_counts(), _hip.conv_i8z_plane_counts()
        assert _same(got, eager)
        # the replay trims by the bits of the input it finds: the rule's rounds and the model's planes for THAT input
        assert ((c1[0] - c0[0], c1[1] - c0[1]), (p1[0] - p0[0], p1[1] - p0[1])) == want[name], (name, c0, c1, p0, p1, want[name])
    assert _hip.device_status()[0] == 0 and _hip.conv_i8_spin_timeouts() == spins
