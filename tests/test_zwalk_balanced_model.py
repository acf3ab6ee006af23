"""The z-walk's balanced deal on the host (tools/debug/zwalk_balanced_model.py; csrc/conv_i8z.inc "THE BALANCED DEAL"), no
GPU: what the model derives from the row bits is what the plan model and the window rule derive from the occupancy bytes, the
deal is a permutation of the jobs with the live ones first, the guard falls back where it says, and the benchmark's batch
gives the figures the design quotes."""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", "debug", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


rule = _tool("zwalk_window_rule")
model = _tool("zwalk_plan_model")
bal = _tool("zwalk_balanced_model")

# (B, Z, X, Y): 256 columns each -- four segments, four with four columns per tile, two segments, a partial last column
SHAPES = [(32, 64, 64, 16), (64, 64, 32, 64), (32, 32, 64, 16), (32, 64, 60, 32)]


def _grids(shape):
    rng = np.random.default_rng(sum(shape))
    B, Z, X, Y = shape
    ground = np.zeros(shape, dtype=bool)
    ground[:, :13] = rng.random((B, 13, X, Y)) < 0.05
    ground[1, :, 3:5, 4:9] = True
    ground[B - 2, :, X - 6:X - 3, 2:6] = True
    sparse = rng.random(shape) < 0.0005
    return {"zero": np.zeros(shape, dtype=bool), "ground_and_towers": ground, "sparse": sparse, "half": rng.random(shape) < 0.5}


def test_the_bit_layout():
    occ = np.zeros((2, 3, 40, 16), dtype=bool)
    occ[1, 2, 0, 5] = occ[1, 2, 31, 0] = occ[1, 2, 32, 15] = occ[0, 0, 39, 3] = True
    rows = bal.row_bits(occ)
    assert rows.shape == (2, 3, 2) and rows.dtype == np.uint32
    assert rows[1, 2, 0] == (1 | 1 << 31) and rows[1, 2, 1] == 1 and rows[0, 0, 1] == 1 << 7 and rows.sum() == (1 | 1 << 31) + 1 + (1 << 7)
    assert np.array_equal(bal.rows_to_bool(rows, 40), occ.any(axis=-1))


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("kH", [1, 2])
def test_liveness_and_rounds_from_the_bits_are_the_bytes(shape, kH):
    B, Z, X, Y = shape
    p = bal.plan(B, Z, X, Y, 0)
    assert p["bal"] == 1
    for name, occ in _grids(shape).items():
        rowsb = bal.rows_to_bool(bal.row_bits(occ), X)
        ran = dead_rounds = 0
        for j in range(p["njobs"]):
            job = model.decode(p, j)[0]
            c, lv, r = bal.job_cost(rowsb, p, job, kH)
            assert lv == model.live(occ, p, job), (name, job)
            assert c == (bal.PLANE_NS * p["PL"] + bal.ROUND_NS * r if lv else bal.FILL_NS) and (lv or r == 0)
            ran += r
        assert ran == rule.counts(occ, kH)[0], name


@pytest.mark.parametrize("shape", SHAPES)
def test_the_deal_is_a_permutation_inside_each_tile(shape):
    B, Z, X, Y = shape
    p = bal.plan(B, Z, X, Y, 0)
    for name, occ in _grids(shape).items():
        rows = bal.row_bits(occ)
        tables = bal.deal(rows, p, 1)
        assert len(tables) == p["grid"]
        assert sorted(j for ids, _ in tables for j in ids) == list(range(p["njobs"])), name
        rowsb = bal.rows_to_bool(rows, X)
        for wg, (ids, nlive) in enumerate(tables):
            c0 = model.job_id(p, wg, 0)
            assert 1 <= len(ids) <= bal.MAX_TILE_JOBS
            assert all(model.decode(p, j)[0][0] == c0 // p["nxt"] for j in ids), "jobs of the workgroup's own tile only"
            lives = [bal.job_cost(rowsb, p, model.decode(p, j)[0], 1)[1] for j in ids]
            assert lives == [True] * nlive + [False] * (len(ids) - nlive)
        if name == "zero" or (name == "half" and X % 8 == 0):   # equal costs: the static sets
            assert all(sorted(ids) == [sg * p["ncol"] + model.job_id(p, wg, 0) for sg in range(p["nseg"])]
                       for wg, (ids, _) in enumerate(tables))
        # never worse than the static deal of the same segments under the same cost
        static = dict(p, bal=0)
        assert bal.cost_us(rows, p, 1).max() <= bal.cost_us(rows, static, 1).max() + 1e-9, name


def test_the_guard():
    assert bal.plan(32, 64, 64, 64, 0)["bal"] == 1 and bal.plan(32, 64, 64, 64, 0)["nseg"] == 4
    assert bal.plan(32, 32, 64, 64, 0)["nseg"] == 2 and bal.plan(32, 32, 64, 64, 0)["bal"] == 1
    for seg in (2, 4):
        assert bal.plan(32, 64, 64, 64, seg)["bal"] == 1 and bal.plan(32, 64, 64, 64, seg)["nseg"] == seg
    assert bal.plan(32, 64, 64, 64, 3)["bal"] == 0                                  # 3 does not divide 64
    assert bal.plan(32, 64, 64, 64, 1)["bal"] == 0 and bal.plan(32, 64, 64, 64, 1)["deal"] == 0
    assert bal.plan(32, 64, 64, 64, 0, bits=False) == dict(model.plan(32, 64, 64, 64, 0), bal=0)   # no bits: today's plan
    assert bal.plan(32, 64, 64, 64, 0, head_only=False)["bal"] == 0 and bal.plan(32, 64, 64, 64, 0, dense=True)["bal"] == 0
    assert bal.plan(5, 32, 16, 16, 0)["bal"] == 0                                   # 10 columns
    assert bal.plan(32, 64, 64, 80, 0)["bal"] == 0                                  # two y tiles
    p = bal.plan(32, 128, 128, 128, 0)                                              # 128^3: as without bits
    assert p["bal"] == 0 and p == dict(model.plan(32, 128, 128, 128, 0), bal=0)
    # columns != workgroups, two y tiles, a partial batch: the plan is the no-bits plan, segment count included
    for B, Z, X, Y, cus in [(31, 64, 64, 64, 256), (64, 64, 64, 64, 256), (16, 64, 64, 64, 256), (32, 64, 64, 64, 304),
                            (32, 64, 64, 80, 256), (5, 32, 16, 16, 256)]:
        for seg in (0, 2, 4):
            assert bal.plan(B, Z, X, Y, seg, cus=cus) == dict(model.plan(B, Z, X, Y, seg, cus=cus), bal=0), (B, Z, X, Y, cus, seg)
    assert model.plan(64, 64, 64, 64, 0)["nseg"] == bal.plan(64, 64, 64, 64, 0)["nseg"] == 2


def test_the_benchmarks_batch():
    """32 synthetic tiles of 100 k points at 64^3: the window rule's 36 899 rounds run of 131 072 (94 173 skipped), the
    four-segment plan's 538 dead jobs of 1024, and the model's busiest workgroup: 66.5 us under the static two-segment deal,
    73.6 under four static segments, below 60 under the balanced four"""
    occ = bal.bench_occ()
    rows = bal.row_bits(occ)
    rowsb = bal.rows_to_bool(rows, 64)
    p = bal.plan(32, 64, 64, 64, 0)
    assert p["bal"] == 1 and p["nseg"] == 4 and p["njobs"] == 1024
    costs = [bal.job_cost(rowsb, p, model.decode(p, j)[0], 1) for j in range(p["njobs"])]
    assert sum(c[2] for c in costs) == 36899 == rule.counts(occ, 1)[0] and rule.counts(occ, 1)[1] == 94173
    dead = sum(not c[1] for c in costs)
    assert dead == 538 == sum(not model.live(occ, p, j) for mine in model.jobs(p) for j in mine)
    two = model.cost(occ, model.plan(32, 64, 64, 64, 0), 1).max()
    four_static = bal.cost_us(rows, bal.plan(32, 64, 64, 64, 4, bits=False), 1).max()
    four = bal.cost_us(rows, p, 1).max()
    print(f"busiest workgroup, modelled us: two static {two:.1f}, four static {four_static:.1f}, four balanced {four:.1f}")
    assert abs(two - 66.5) < 0.05 and abs(four_static - 73.6) < 0.05 and four < 60.0
