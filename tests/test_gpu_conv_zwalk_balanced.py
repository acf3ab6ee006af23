"""The z-walk's balanced deal (csrc/conv_i8z.inc "THE BALANCED DEAL", sn_conv_bank_prepared_rows): with the occupancy's row
bits a head-only launch cuts its columns into four z segments (two below Z = 64) and the workgroups of a tile share the
tile's jobs by cost.  Nothing about the results may show it: every call writes into a buffer pre-filled with NaN bits and is
compared ON THE RAW BITS with the same call without bits under conv_i8z_segments = 1 (whole columns) and under
conv_i8z_dense = 1; the round counters must be what the numpy rule predicts, and the deal the launch reports (plan_out) must
be the numpy model's (tools/debug/zwalk_balanced_model.py).  Then the bits' way through the pipeline: the voxel stage writes
them, they ride on the occupancy tensor, and they are dropped the moment that tensor is written to."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import scene_net_amd as sna
from scene_net_amd import _hip
from scene_net_amd.synthetic import synthetic_tile

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
GUARDED = (5, 32, 16, 16)                    # 10 columns: the static deal
GUARDED64 = (16, 64, 64, 16)                 # Z = 64 with 128 columns: the static deal of TWO segments, as without bits
OFF = (GUARDED, GUARDED64)


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


def _walk(x, bank, lam, prep, rows=None, dt=torch.float32, served=True, out=None, plan=None):
    """the head-only prepared call into a buffer full of NaN bits -> (out, (rounds run, skipped))"""
    B, _, Z, X, Y = x.shape
    if out is None:
        out = torch.full((B, 1, Z, X, Y), float("nan"), dtype=dt, device=x.device)
    c0 = _hip.conv_i8z_round_counts()
    rc = _hip.load().sn_conv_bank_prepared_rows(
        x.data_ptr(), _hip.SN_OCC8, bank.data_ptr(), lam.data_ptr(), prep.data_ptr(), B, Z, X, Y, bank.shape[0], 9, 9, 9,
        None, out.data_ptr(), _hip.SN_F32 if dt == torch.float32 else _hip.SN_F64, torch.cuda.current_stream().cuda_stream,
        int(served), None if rows is None else rows.data_ptr(), None if plan is None else plan.data_ptr())
    assert rc == 0, rc
    c1 = _hip.conv_i8z_round_counts()
    return out, (c1[0] - c0[0], c1[1] - c0[1])


def _check(occ, bank, lam, prep, rows=None, dt=torch.float32, variants=(2,), groups=1, served=True, seg=0, moved=None):
    """occ (host, bool) with bits (the true ones unless `rows`, a host uint32 array, is given): equal to whole columns
    without bits and to the dense walk bit for bit, no sentinel left, the rule's round counts, the model's deal -> out"""
    dev = bank.device
    x = occ.to(dev)
    B, _, Z, X, Y = occ.shape
    rows_h = bal.row_bits(occ.numpy()) if rows is None else rows
    rows_d = torch.from_numpy(rows_h.view(np.int32)).to(dev)
    if rows is None:
        assert torch.equal(_hip.row_bits_of(x), rows_d), "row_bits_of disagrees with the numpy layout"
    p = bal.plan(B, Z, X, Y, seg, cus=_cus())
    out = None
    for v in variants:
        want = rule.counts(occ.numpy(), KH[v])
        plan = torch.full((_cus(), 65), -1, dtype=torch.int32, device=dev)
        with _hip.options(conv_i8z_variant=v):
            with _hip.options(conv_i8z_segments=seg):
                out, cnt = _walk(x, bank, lam, prep, rows_d, dt, served, plan=plan)
            with _hip.options(conv_i8z_segments=1):
                out_p, cnt_p = _walk(x, bank, lam, prep, None, dt, served)
            with _hip.options(conv_i8z_dense=1):
                out_d, cnt_d = _walk(x, bank, lam, prep, rows_d, dt, served)
        print(f"variant {v}: bal {p['bal']} segments {p['nseg']} rounds {cnt} whole columns {cnt_p} dense {cnt_d} rule {want}")
        assert not bool(torch.isnan(out).any()), (v, "an output was not written")
        assert _same(out, out_p) and _same(out, out_d), v
        assert cnt == cnt_p == (groups * want[0], groups * want[1]), (v, cnt, cnt_p, want)
        assert cnt_d == (groups * (want[0] + want[1]), 0), (v, cnt_d)
        got = plan.cpu().numpy()
        if p["bal"]:
            tables = bal.deal(rows_h, p, KH[v])
            seen = []
            for wg, (ids, _nlive) in enumerate(tables):
                assert got[wg, 0] == len(ids) and list(got[wg, 1:1 + len(ids)]) == ids, (v, wg, got[wg, :10], ids)
                seen += ids
            assert sorted(seen) == list(range(p["njobs"])), "every job is dealt exactly once"
            if moved is not None:
                static = [[sg * p["ncol"] + bal.pm.job_id(p, wg, 0) for sg in range(p["nseg"])] for wg in range(p["grid"])]
                assert ([sorted(t[0]) for t in tables] != [sorted(s) for s in static]) == moved
        else:
            assert bool((got == -1).all()), "the static deal reports no plan"
    assert _hip.device_status()[0] == 0
    return out


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


@pytest.mark.parametrize("B,Z,X,Y", SHAPES + [GUARDED, GUARDED64])
def test_all_zero_every_job_is_dead(dev, bank16, B, Z, X, Y):
    bank, lam, prep = bank16
    occ = torch.zeros((B, 1, Z, X, Y), dtype=torch.bool)
    assert bal.plan(B, Z, X, Y, 0, cus=_cus())["bal"] == int((B, Z, X, Y) not in OFF)
    out = _check(occ, bank, lam, prep, variants=(0, 1, 2), moved=False if (B, Z, X, Y) not in OFF else None)
    assert bool((_bits(out) == 0).all())


@pytest.mark.parametrize("B,Z,X,Y", SHAPES + [GUARDED, GUARDED64])
def test_ground_and_full_height_columns_move_jobs(dev, bank16, B, Z, X, Y):
    bank, lam, prep = bank16
    occ = _ground_and_towers(B, Z, X, Y, Z + X)
    p = bal.plan(B, Z, X, Y, 0, cus=_cus())
    assert p["bal"] == int((B, Z, X, Y) not in OFF) and (not p["bal"] or p["nseg"] == (4 if Z == 64 else 2))
    if (B, Z, X, Y) == GUARDED64:   # off the guard the bits change nothing: the plan is the no-bits plan, two segments
        assert p == dict(bal.pm.plan(B, Z, X, Y, 0, cus=_cus()), bal=0) and p["nseg"] == 2
    out = _check(occ, bank, lam, prep, variants=(0, 1, 2) if (B, Z, X, Y) == SHAPES[0] else (2,),
                 moved=True if p["bal"] and Z == 64 else None)
    assert bool((out != 0).any())
    _check(occ, bank, lam, prep, served=False)


@pytest.mark.parametrize("B,Z,X,Y", [SHAPES[1], GUARDED])
def test_random_half_occupancy_nothing_is_dead(dev, bank16, B, Z, X, Y):
    bank, lam, prep = bank16
    g = torch.Generator().manual_seed(50)
    occ = torch.rand((B, 1, Z, X, Y), generator=g) < 0.5
    _check(occ, bank, lam, prep, moved=False if (B, Z, X, Y) != GUARDED else None)


@pytest.mark.parametrize("B,Z,X,Y", SHAPES)
def test_sparse_random_every_cost_differs(dev, bank16, B, Z, X, Y):
    """0.05 % set, up to the grid's first and last planes and rows: a deal that is sensitive to every job's round count"""
    bank, lam, prep = bank16
    g = torch.Generator().manual_seed(B + Z)
    occ = torch.rand((B, 1, Z, X, Y), generator=g) < 0.0005
    occ[:, 0, 0, ::7, 3] = True
    occ[:, 0, Z - 1, 1::9, 5] = True
    _check(occ, bank, lam, prep, variants=(0, 2), moved=True)


def test_one_voxel_at_each_face_of_a_jobs_region_and_one_step_outside(dev, bank16):
    """(32, 32, 64, 16), LZ = 16: the job (tile 3, x0 = 24, zs = 16) for the lower z face and the x faces, (3, 24, 0) for the
    upper z face; a voxel ON a face makes the job live, one step outside leaves it dead"""
    bank, lam, prep = bank16
    B, Z, X, Y = SHAPES[2]
    p = bal.plan(B, Z, X, Y, 0, cus=_cus())
    assert p["bal"] == 1 and p["LZ"] == 16
    lo, up = (3, 24, 0, 16), (3, 24, 0, 0)
    cases = [(lo, (12, 30, 7), True), (lo, (11, 30, 7), False), (up, (19, 30, 7), True), (up, (20, 30, 7), False),
             (lo, (20, 20, 0), True), (lo, (20, 19, 15), False), (lo, (20, 35, 15), True), (lo, (20, 36, 0), False)]
    for job, (z, xx, y), is_live in cases:
        occ = torch.zeros((B, 1, Z, X, Y), dtype=torch.bool)
        occ[3, 0, z, xx, y] = True
        rowsb = bal.rows_to_bool(bal.row_bits(occ.numpy()), X)
        assert bal.job_cost(rowsb, p, job, 1)[1] == is_live == bal.pm.live(occ[:, 0].numpy(), p, job), (job, z, xx, y)
        out = _check(occ, bank, lam, prep)
        assert bool((out != 0).any())


@pytest.mark.parametrize("B,Z,X,Y", [SHAPES[0], GUARDED])
def test_a_superset_of_the_bits_gives_the_same_output(dev, bank16, B, Z, X, Y):
    bank, lam, prep = bank16
    occ = _ground_and_towers(B, Z, X, Y, 77)
    true_rows = bal.row_bits(occ.numpy())
    ref = _check(occ, bank, lam, prep)
    rng = np.random.default_rng(5)
    extra = rng.integers(0, 2 ** 32, size=true_rows.shape, dtype=np.uint64).astype(np.uint32)
    extra &= rng.integers(0, 2 ** 32, size=true_rows.shape, dtype=np.uint64).astype(np.uint32)
    if X < 32:
        extra &= np.uint32((1 << X) - 1)
    for rows in (np.full_like(true_rows, (1 << min(X, 32)) - 1 if X < 32 else 0xffffffff), true_rows | extra):
        assert _same(_check(occ, bank, lam, prep, rows=rows), ref)


def test_fp64_head(dev, bank16):
    bank, lam, prep = bank16
    _check(_ground_and_towers(*SHAPES[1], 64), bank, lam, prep, dt=torch.float64, variants=(0, 2), moved=True)


@pytest.mark.parametrize("dt", [torch.float32, torch.float64], ids=["fp32", "fp64"])
def test_two_groups_accumulate_into_one_head(dev, dt):
    """G = 20: the second group's launch loads what the first stored, adds and activates (head & 1) -- in its filled jobs too"""
    bank, lam = _bank(20, 7).to(dev), _lam(20, 8).to(dev)
    prep = _hip.conv_bank_prep(bank)
    occ = _ground_and_towers(*SHAPES[1], 20)
    _hip.conv_bank(occ.to(dev), bank, lam, prep=prep)
    _check(occ, bank, lam, prep, dt=dt, groups=2, moved=True)


def test_a_nan_coefficient_fills_nothing_and_takes_the_static_deal(dev, bank16):
    bank, lam, _ = bank16
    bank, lam = bank.clone(), lam.clone()
    lam[5] = float("nan")
    prep = _hip.conv_bank_prep(bank)
    B, Z, X, Y = SHAPES[1]
    occ = _ground_and_towers(B, Z, X, Y, 9)
    x = occ.to(dev)
    rows = _hip.row_bits_of(x)
    p = bal.plan(B, Z, X, Y, 0, cus=_cus())
    plan = torch.full((_cus(), 65), -1, dtype=torch.int32, device=dev)
    out, cnt = _walk(x, bank, lam, prep, rows, served=False, plan=plan)
    with _hip.options(conv_i8z_segments=1):
        out_p, cnt_p = _walk(x, bank, lam, prep, None, served=False)
    assert _same(out, out_p) and cnt == cnt_p == (sum(rule.counts(occ.numpy(), 1)), 0)
    assert bool(torch.isnan(out).all())
    got = plan.cpu().numpy()
    for wg in range(p["grid"]):
        assert list(got[wg, :1 + p["nseg"]]) == [p["nseg"]] + [bal.pm.job_id(p, wg, k) for k in range(p["nseg"])]
    assert _hip.device_status()[0] == 0


def test_a_captured_call_replays(dev, bank16):
    bank, lam, prep = bank16
    B, Z, X, Y = SHAPES[1]
    occ = _ground_and_towers(B, Z, X, Y, 11)
    x = occ.to(dev)
    eager, _ = _walk(x, bank, lam, prep, _hip.row_bits_of(x))
    got = torch.full_like(eager, float("nan"))
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
    for _ in range(3):
        got.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert _same(got, eager)
    assert _hip.device_status()[0] == 0


# ------------------------------------------------------------------------------------------------ through the pipeline
@pytest.fixture(scope="module")
def small_batch(dev):
    tiles, labels = zip(*[synthetic_tile(t, 3000) for t in range(32)])
    return sna.PointBatch.from_tiles(tiles, labels, device=dev)


@pytest.mark.parametrize("dims", [(64, 64, 64), (32, 32, 32), (24, 16, 8)], ids=["64", "32", "24x16x8"])
@pytest.mark.parametrize("onepass", [1, 0], ids=["onepass", "two_kernels"])
@pytest.mark.parametrize("rider", [False, True], ids=["plain", "rider"])
def test_the_voxel_stage_writes_the_row_bits(dev, small_batch, dims, onepass, rider):
    torch.manual_seed(1)
    model = sna.SceneNet({"cy": 2, "cone": 1, "neg": 1}, (9, 9, 9)).to(dev)
    pipe = sna.ScenePipeline(model, dims, keep_labels=[15])
    with _hip.options(voxel_onepass=onepass), torch.no_grad():
        grids = pipe.voxelize(small_batch, bank_rider=model.bank_rider(dev) if rider else None)
    assert grids.row_bits is not None and grids.row_bits.shape == (32, dims[2], (dims[0] + 31) // 32)
    true = _hip.row_bits_of(grids.occ)
    clean = grids.flags == 0                    # (a flagged tile keeps a superset: below)
    assert bool(grids.occ.any()) and bool(clean.any())
    assert torch.equal(grids.row_bits[clean], true[clean]) and bool(((grids.row_bits & true) == true).all())
    assert _hip.rows_for(grids.occ) is grids.row_bits


def test_a_flagged_tile_keeps_a_superset(dev):
    """8 x 32 x 8 voxels and 40 k points: no (z, x) row is empty, the flag goes up and the exact fallback rewrites the tile"""
    rng = np.random.default_rng(3)
    tiles = [rng.random((40_000, 3)) * 10.0 for _ in range(2)]
    batch = sna.PointBatch.from_tiles(tiles, [np.zeros(40_000) for _ in range(2)], device=dev)
    grids = sna.voxelization.voxelize_batch(batch, (8, 32, 8), occ_dtype=torch.bool)
    rows, true = grids.row_bits, _hip.row_bits_of(grids.occ)
    print("flags", grids.flags.tolist(), "rows set", int((rows != 0).sum()), int((true != 0).sum()))
    assert int(grids.flags.sum()) == 2, "the tiles were meant to be full"
    assert rows is not None and bool(((rows & true) == true).all())


def test_the_bits_ride_on_the_occupancy_and_die_with_a_write(dev, small_batch, monkeypatch):
    handed = []                                 # what conv_bank's look at the tensor gave, call by call
    rows_for = _hip.rows_for
    monkeypatch.setattr(_hip, "rows_for", lambda x: handed.append(rows_for(x)) or handed[-1])
    torch.manual_seed(2)
    model = sna.SceneNet({"cy": 2, "cone": 1, "neg": 1}, (9, 9, 9)).to(dev)
    pipe = sna.ScenePipeline(model, (64, 64, 64), keep_labels=[15])
    with torch.no_grad():
        grids = pipe.voxelize(small_batch)
        bank, prep = model.compute_bank_prepared(dev)
        lam = model.effective_lambdas(dev)
        del handed[:]                           # (the voxel stage looked too)
        out = model.contract_prepared(grids.occ, bank, lam, prep)[1]
        assert len(handed) == 1 and handed[0] is grids.row_bits
        # the deal the launch made is the model's, from these bits
        plan = torch.full((_cus(), 65), -1, dtype=torch.int32, device=dev)
        out2 = _hip.conv_bank(grids.occ, bank, lam, prep=prep, plan_out=plan)[1]
        p = bal.plan(32, 64, 64, 64, 0, cus=_cus())
        if p["bal"]:
            tables = bal.deal(grids.row_bits.cpu().numpy().view(np.uint32), p, KH[_hip.get_option("conv_i8z_variant")])
            got = plan.cpu().numpy()
            for wg, (ids, _) in enumerate(tables):
                assert list(got[wg, :1 + len(ids)]) == [len(ids)] + ids, (wg, got[wg, :10], ids)
        with _hip.options(conv_i8z_segments=1):
            ref = _hip.conv_bank(grids.occ.clone(), bank, lam, prep=prep)[1]
        assert _same(out, ref) and _same(out2, ref)
        # a view, a clone and a written tensor carry no bits
        assert rows_for(grids.occ.clone()) is None and rows_for(grids.occ[:]) is None
        grids.occ[0, 0, 0, 0, 0] ^= True
        assert rows_for(grids.occ) is None
        del handed[:]
        got = model.contract_prepared(grids.occ, bank, lam, prep)[1]
        assert handed == [None]
        with _hip.options(conv_i8z_segments=1):
            ref = _hip.conv_bank(grids.occ.clone(), bank, lam, prep=prep)[1]
        assert _same(got, ref)
    assert _hip.device_status()[0] == 0
