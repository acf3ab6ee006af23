"""The z-walk's lean ticket (csrc/conv_i8z.inc, "THE TICKET'S VERDICT FIRST"; the contraction of SceneNet.forward,
core/models/SCENE_Net.py:322-339): a ticket whose rounds are all empty stores its rows of + 0.0 from one row address -- both
rows in one wider store where they are contiguous in memory -- and the tile bases are formed once per job.  Nothing about the
results may show it.  The yardstick is that of test_gpu_conv_zwalk_skip.py: equality ON THE RAW BITS with the same call under
sn_set_option("conv_i8z_dense", 1) and with sn_conv_bank without a blob (the folded tile kernel), on the three
conv_i8z_variant shapes, through sn_conv_bank_prepared and _served.  Every walk call here writes into a buffer pre-filled with
a sentinel (NaN bits), so that a row the path forgot shows, and the round counters must be what the numpy rule predicts."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from scene_net_amd import _hip

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("zwalk_window_rule", os.path.join(ROOT, "tools", "debug", "zwalk_window_rule.py"))
rule = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rule)

VARIANTS = (0, 1, 2)
KH = {0: 2, 1: 1, 2: 1}                      # x-rows per round of each variant


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


def _walk(x, bank, lam, prep, dt, served):
    """the head-only prepared call into a buffer full of NaN bits -> (out, (rounds run, skipped))"""
    B, _, Z, X, Y = x.shape
    out = torch.full((B, 1, Z, X, Y), float("nan"), dtype=dt, device=x.device)
    fn = _hip.load().sn_conv_bank_prepared_served if served else _hip.load().sn_conv_bank_prepared
    c0 = _hip.conv_i8z_round_counts()
    rc = fn(x.data_ptr(), _hip.SN_OCC8, bank.data_ptr(), lam.data_ptr(), prep.data_ptr(), B, Z, X, Y, bank.shape[0], 9, 9, 9,
            None, out.data_ptr(), _hip.SN_F32 if dt == torch.float32 else _hip.SN_F64, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    c1 = _hip.conv_i8z_round_counts()
    return out, (c1[0] - c0[0], c1[1] - c0[1])


def _everywhere(occ, bank, lam, dt=torch.float32, groups=1):
    """occ (host, bool) on the three variants through both entries: the default call equals its dense twin and the folded
    tile kernel bit for bit, leaves no sentinel, and reports the rounds the rule predicts -> out"""
    x = occ.to(bank.device)
    ref = _hip.conv_bank(x, bank, lam, out_dtype=dt)[1]
    assert not bool(torch.isnan(ref).any())
    prep = _hip.conv_bank_prep(bank)
    _hip.conv_bank(x, bank, lam, prep=prep)       # (the verdict the served entry rests on: these banks are served)
    for v in VARIANTS:
        want = rule.counts(occ.numpy(), KH[v])
        with _hip.options(conv_i8z_variant=v):
            for served in (False, True):
                out, cnt = _walk(x, bank, lam, prep, dt, served)
                with _hip.options(conv_i8z_dense=1):
                    out_d, cnt_d = _walk(x, bank, lam, prep, dt, served)
                assert not bool(torch.isnan(out).any()), (v, served, "a row was not written")
                assert _same(out, out_d) and _same(out, ref), (v, served)
                assert cnt == (groups * want[0], groups * want[1]), (v, served, cnt, want)
                assert cnt_d == (groups * (want[0] + want[1]), 0), (v, served, cnt_d)
    assert _hip.device_status()[0] == 0
    return ref


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def bank16(dev):
    return _bank(16, 3).to(dev), _lam(16, 4).to(dev)


@pytest.mark.parametrize("X", [9, 11])
def test_a_tickets_second_row_outside_the_grid(dev, bank16, X):
    """X = 9, 11: the two-row ticket of rows (8, 9) / (10, 11) has its second row outside the grid.  The ticket of plane z = 7
    (tile 0) and of plane 15 (tile 0's last) is empty, while the row that FOLLOWS its first row in memory -- x = 0 of plane 8,
    and tile 1's first row -- holds non-zero results: a store one row too wide would show."""
    bank, lam = bank16
    shape = (2, 1, 16, X, 64)
    occ = torch.zeros(shape, dtype=torch.bool)
    occ[0, 0, 8, 0, 30] = True
    occ[1, 0, 0, 0, 30] = True
    if X == 11:
        occ[0, 0, 8, 1, 30] = True              # (row 10's window reaches down to x = 6: still empty)
    out = _everywhere(occ, bank, lam)
    assert bool((out[0, 0, 8, 0] != 0).any()) and bool((out[1, 0, 0, 0] != 0).any())
    assert bool((_bits(out[0, 0, 7, X - 1]) == 0).all()) and bool((_bits(out[0, 0, 15, X - 1]) == 0).all())


@pytest.mark.parametrize("Y", [16, 32, 48, 128])
def test_partial_y_tiles_and_two_y_tiles(dev, bank16, Y):
    """Y = 16, 32, 48: a partial y tile (the wide store covers 2 Y values, not 128).  Y = 128: two y tiles, so the rows of a
    column are not contiguous and the wide store must not be taken -- the voxel sits in y tile 1 only, y tile 0's tickets are
    all empty next to non-zero values of the same rows"""
    bank, lam = bank16
    shape = (1, 1, 16, 8, Y)
    occ = torch.zeros(shape, dtype=torch.bool)
    occ[0, 0, 3, 5, Y - 6 if Y < 128 else 100] = True
    out = _everywhere(occ, bank, lam)
    assert bool((out[0, 0, 3, 5] != 0).any()) and bool((_bits(out[0, 0, 12]) == 0).all())
    if Y == 128:
        assert rule.counts(occ.numpy(), 1)[1] >= 16 * 8      # (y tile 0 runs nothing)
        assert bool((out[0, 0, 3, :, 96:105] != 0).any()) and bool((_bits(out[0, 0, :, :, :64]) == 0).all())


def test_more_columns_than_workgroups(dev, bank16):
    """300 columns of one tile each: a workgroup walks two jobs of different tiles (the per-job bases); the first tile, one in
    the middle and the last carry one voxel each"""
    bank, lam = bank16
    shape = (300, 1, 16, 8, 16)
    occ = torch.zeros(shape, dtype=torch.bool)
    for b, z, xx, y in ((0, 2, 1, 3), (150, 8, 4, 9), (299, 15, 7, 15)):
        occ[b, 0, z, xx, y] = True
    out = _everywhere(occ, bank, lam)
    busy = (out != 0).flatten(1).any(1).cpu()
    assert busy.nonzero().flatten().tolist() == [0, 150, 299]


def test_fp64_head_over_two_groups(dev):
    """G = 20: the second group's launch adds to what the first stored (head & 1) and applies the head.  A ticket that is empty
    is empty in both groups: group 0 stores the constant, group 1 loads, adds and activates.  fp64 output (the wide store is
    16 bytes per lane), once sparse and once all-empty -- with `out` pre-filled with NaN bits, which group 0 must have
    replaced everywhere before group 1 adds to it"""
    bank, lam = _bank(20, 7).to(dev), _lam(20, 8).to(dev)
    shape = (2, 1, 20, 20, 48)
    occ = torch.zeros(shape, dtype=torch.bool)
    torch.manual_seed(71)
    occ[:, :, 12:, 10:] = torch.rand((2, 1, 8, 10, 48)) < 0.2
    assert rule.counts(occ.numpy(), 1)[1] > 0
    for dt in (torch.float64, torch.float32):
        _everywhere(occ, bank, lam, dt=dt, groups=2)
    out = _everywhere(torch.zeros(shape, dtype=torch.bool), bank, lam, dt=torch.float64, groups=2)
    assert bool((_bits(out) == 0).all())


@pytest.mark.parametrize("xx,which", [(0, "first"), (13, "second")])
@pytest.mark.parametrize("dt", [torch.float32, torch.float64], ids=["fp32", "fp64"])
def test_one_round_of_a_ticket_empty_the_other_not(dev, bank16, xx, which, dt):
    """variant 2's tickets hold the x-rows (2 k, 2 k + 1).  A voxel at x = 0 reaches rows 0 .. 4: of the ticket (4, 5) only its
    first round runs; a voxel at x = 13 reaches rows 9 .. 17: of the ticket (8, 9) only its second.  The output buffer is
    pre-filled, so the empty round's row must have been written"""
    bank, lam = bank16
    shape = (1, 1, 12, 24, 64)
    occ = torch.zeros(shape, dtype=torch.bool)
    occ[0, 0, 6, xx, 40] = True
    out = _everywhere(occ, bank, lam, dt=dt)
    lone, empty = (4, 5) if which == "first" else (9, 8)
    assert bool((out[0, 0, 6, lone] != 0).any()) and bool((_bits(out[0, 0, 6, empty]) == 0).all())
