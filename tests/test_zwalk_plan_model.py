"""The z-walk's dealt plan and its dead jobs on the host (tools/debug/zwalk_plan_model.py; csrc/conv_i8z.inc "DEAD JOBS"), no
GPU: a dead job has no round the window rule (tools/debug/zwalk_window_rule.py) would run, the jobs cover every output exactly
once, the dealt numbering is a permutation of (column, segment), and the option that selects the plan is in the table."""
import importlib.util
import os
import re

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

# (B, Z, X, Y, segments): 64^3 with B = 32 (the headline: 256 columns, one per workgroup), a last segment shorter (Z = 33), a
# partial column in x (X = 9), two y tiles, three columns (the shift is not half), more jobs than workgroups, 3 and 4 segments
# (auto -- segments 0 -- deals only where the dense plan walks whole columns, i.e. with about a column per workgroup or more)
SHAPES = [(32, 64, 64, 64, 0), (3, 33, 16, 64, 2), (2, 32, 9, 64, 2), (2, 32, 16, 80, 2), (2, 32, 24, 64, 2),
          (150, 16, 16, 16, 2), (2, 32, 16, 64, 3), (2, 32, 16, 64, 4), (2, 33, 9, 80, 2), (128, 32, 16, 16, 0)]


def _sparse(shape, seed):
    """a few small clusters in the lowest quarter of z: the upper segments are dead, some lower ones live"""
    rng = np.random.default_rng(seed)
    B, Z, X, Y = shape
    occ = np.zeros(shape, dtype=bool)
    for _ in range(max(2, B // 4)):
        b, z, x, y = rng.integers(B), rng.integers(Z // 4), rng.integers(X), rng.integers(Y)
        blob = rng.random((min(3, Z - z), min(3, X - x), min(5, Y - y))) < 0.5
        occ[b, z:z + 3, x:x + 3, y:y + 5] |= blob
    return occ


@pytest.mark.parametrize("B,Z,X,Y,seg", SHAPES)
def test_the_dealt_numbering_is_a_permutation_and_covers_every_output_once(B, Z, X, Y, seg):
    p = model.plan(B, Z, X, Y, seg)
    assert p["deal"] == 1 and p["fill_dead"] == 1 and p["shift"] == max(1, p["nxt"] // p["nseg"])
    keys = [model.decode(p, j)[1] for j in range(p["njobs"])]
    assert len(set(keys)) == p["njobs"] == B * p["nyt"] * p["nxt"] * p["nseg"]
    assert set(keys) == {(b, yt, xt, sg) for b in range(B) for yt in range(p["nyt"]) for xt in range(p["nxt"])
                         for sg in range(p["nseg"])}
    per_wg = model.jobs(p)
    assert len(per_wg) == p["grid"] and sum(len(m) for m in per_wg) == p["njobs"] and max(len(m) for m in per_wg) <= 256
    cover = np.zeros((B, Z, X, Y), dtype=np.int32)
    for mine in per_wg:
        for (b, x0, y0, zs) in mine:
            cover[b, zs:zs + p["LZ"], x0:x0 + 8, y0:y0 + 64] += 1
    assert cover.min() == 1 and cover.max() == 1
    if p["nseg"] == 2 and p["nxt"] >= 2 and p["grid"] == p["ncol"]:
        # one column's worth of workgroups: a workgroup's two segments come from different columns of the same (b, y tile)
        for mine in per_wg:
            (b0, x0, y0, z0), (b1, x1, y1, z1) = mine
            assert (b0, y0) == (b1, y1) and x0 != x1 and z0 != z1


@pytest.mark.parametrize("B,Z,X,Y,seg", SHAPES[1:])
@pytest.mark.parametrize("kH", [1, 2])
def test_a_dead_job_has_no_round_that_would_run(B, Z, X, Y, seg, kH):
    p = model.plan(B, Z, X, Y, seg)
    for seed in (1, 2, 3):
        occ = _sparse((B, Z, X, Y), seed)
        runs = model.run_map(occ, kH)
        ran = total = dead = 0
        for mine in model.jobs(p):
            for job in mine:
                r, t = model.job_rounds(runs, p, job, kH)
                ran += r
                total += t
                if not model.live(occ, p, job):
                    dead += 1
                    assert r == 0, job
                else:
                    assert r > 0, job      # the region is exactly the union of the rounds' windows: a live job runs a round
        assert (ran, total - ran) == rule.counts(occ, kH)      # the map's sums are the rule's, over the jobs once each
        assert 0 < dead < p["njobs"]


def test_auto_takes_the_dealt_plan_only_where_the_issue_says():
    assert model.plan(32, 64, 64, 64, 0)["deal"] == 1 and model.plan(32, 64, 64, 64, 0)["shift"] == 4
    assert model.plan(32, 64, 64, 64, 1)["deal"] == 0
    assert model.plan(32, 64, 64, 64, 0, head_only=False)["deal"] == 0          # the activations form
    assert model.plan(32, 64, 64, 64, 0, dense=True)["deal"] == 0
    assert model.plan(32, 64, 64, 64, 2, dense=True)["deal"] == 0
    assert model.plan(128, 24, 16, 64, 0)["deal"] == 0 and model.plan(128, 32, 16, 64, 0)["deal"] == 1   # Z < 32
    assert model.plan(256, 32, 8, 64, 0)["deal"] == 0                           # one column in x
    assert model.plan(2, 16, 16, 64, 2)["deal"] == 1 and model.plan(2, 16, 16, 64, 2)["LZ"] == 8
    assert model.plan(2, 16, 16, 64, 3)["deal"] == 0                            # a segment would have fewer than 8 planes
    assert model.plan(2, 32, 16, 64, 0)["deal"] == 0                            # the dense plan already cuts these columns
    assert model.plan(2, 32, 24, 64, 2)["shift"] == 1 and model.plan(2, 32, 8, 64, 2)["shift"] == 1
    p = model.plan(32, 128, 128, 128, 0)
    assert p["deal"] == 1 and p["njobs"] == 2048 and p["shift"] == 8


def test_cost_model_on_a_hand_made_grid():
    p1, p2 = model.plan(1, 32, 16, 64, 1, cus=2), model.plan(1, 32, 16, 64, 0, cus=2)
    occ = np.zeros((1, 32, 16, 64), dtype=bool)
    assert np.allclose(model.cost(occ, p1), 3.2 + 0.52 * 40) and np.allclose(model.cost(occ, p2), 3.2)
    occ[0, 2, 2, 30] = True                  # rows 0 .. 6 of column 0, planes 0 .. 6: 49 rounds, one live job
    t1, t2 = model.cost(occ, p1), model.cost(occ, p2)
    assert np.allclose(sorted(t1), [3.2 + 0.52 * 40, 3.2 + 0.52 * 40 + 0.122 * 49])
    assert np.allclose(sorted(t2), [3.2, 3.2 + 0.52 * 24 + 0.122 * 49])


def test_the_option_is_documented_and_in_the_table():
    header = open(os.path.join(ROOT, "include", "scenenet_hip.h")).read()
    assert '"conv_i8z_segments" (0 .. 4, default 0)' in header
    table = open(os.path.join(ROOT, "scene-net_amd", "csrc", "cabi.hip")).read()
    enum = open(os.path.join(ROOT, "scene-net_amd", "csrc", "common.h")).read()
    assert re.search(r'\{"conv_i8z_segments",\s+nullptr,\s+0,\s+0,\s+0,\s+4,\s+false\}', table)
    names = re.findall(r'^\s+\{"(\w+)",', table, flags=re.M)
    kopts = re.findall(r"^\s+kOpt(\w+),", enum, flags=re.M)
    assert len(names) == len(kopts) and names.index("conv_i8z_segments") == kopts.index("ConvI8zSegments")


def test_the_option_round_trips():
    import json, subprocess, sys, textwrap
    from scene_net_amd import _hip
    p = subprocess.run([sys.executable, "-c", textwrap.dedent("""
        import ctypes, json, sys
        lib = ctypes.CDLL(sys.argv[1])
        lib.sn_set_option.argtypes = [ctypes.c_char_p, ctypes.c_int]
        lib.sn_get_option.argtypes = [ctypes.c_char_p]
        name = b"conv_i8z_segments"
        seen = [lib.sn_get_option(name)]
        for v in (1, 4, 5, -1, 2, 0):
            seen.append((lib.sn_set_option(name, v), lib.sn_get_option(name)))
        print(json.dumps(seen))"""), _hip.LIB_PATH], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    got = json.loads(p.stdout.strip().splitlines()[-1])
    assert got == [0, [0, 1], [0, 4], [-1, 4], [-1, 4], [0, 2], [0, 0]]
