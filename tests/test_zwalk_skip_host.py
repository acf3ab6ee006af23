"""The host side of the z-walk's empty-window skip (csrc/conv_i8z.inc, "EMPTY WINDOWS"), no GPU: the option
"conv_i8z_dense", the counter's symbol, and the numpy restatement of the window rule (tools/debug/zwalk_window_rule.py)
that the GPU tests predict the counter with, on hand-made grids."""
import importlib.util
import json
import os
import re
import subprocess
import sys
import textwrap

import numpy as np

from scene_net_amd import _hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("zwalk_window_rule", os.path.join(ROOT, "tools", "debug", "zwalk_window_rule.py"))
rule = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rule)

_LIB = """
import ctypes, json, sys
lib = ctypes.CDLL(sys.argv[1])
lib.sn_set_option.argtypes = [ctypes.c_char_p, ctypes.c_int]
lib.sn_get_option.argtypes = [ctypes.c_char_p]
lib.sn_last_error.restype = ctypes.c_char_p
"""


def _child(body):
    p = subprocess.run([sys.executable, "-c", _LIB + textwrap.dedent(body), _hip.LIB_PATH], capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 0, p.stderr
    return json.loads(p.stdout.strip().splitlines()[-1])


# ------------------------------------------------------------------------------------------------------- the option
def test_dense_option_default_and_round_trip():
    got = _child("""
        name = b"conv_i8z_dense"
        seen = [lib.sn_get_option(name)]
        for v in (1, 0, 5, 0, -3, 0):
            seen.append((lib.sn_set_option(name, v), lib.sn_get_option(name)))
        print(json.dumps(seen))""")
    assert got[0] == 0                                       # the skip is on by default
    assert got[1:] == [[0, v] for v in (1, 0, 1, 0, 1, 0)]   # a switch: any value != 0 is stored as 1


def test_dense_option_through_the_binding():
    p = subprocess.run([sys.executable, "-c", textwrap.dedent("""
        import json, sys
        sys.path.insert(0, sys.argv[1])
        from scene_net_amd import _hip
        seen = [_hip.get_option("conv_i8z_dense")]
        with _hip.options(conv_i8z_dense=1):
            seen.append(_hip.get_option("conv_i8z_dense"))
        seen.append(_hip.get_option("conv_i8z_dense"))
        print(json.dumps(seen))"""), ROOT], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    assert json.loads(p.stdout.strip().splitlines()[-1]) == [0, 1, 0]


def test_the_option_is_documented_and_in_the_table():
    header = open(os.path.join(ROOT, "include", "scenenet_hip.h")).read()
    assert '"conv_i8z_dense" (switch, default 0)' in header
    table = open(os.path.join(ROOT, "scene-net_amd", "csrc", "cabi.hip")).read()
    enum = open(os.path.join(ROOT, "scene-net_amd", "csrc", "common.h")).read()
    assert re.search(r'\{"conv_i8z_dense",\s+nullptr,\s+0,\s+0,\s+0,\s+1,\s+true\}', table)
    # the table's order is the enum's: the new entry is the last of both
    assert re.search(r"kOptConvI8zDense,\s+kOptCount", enum)
    assert table.index('"conv_i8z_dense"') > table.index('"conv_i8z_inject_fault"')


# ------------------------------------------------------------------------------------------------------- the counter
def test_round_counts_symbol_is_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "scenenet_hip.h")).read()
    assert re.search(r"int sn_conv_i8z_round_counts\(unsigned long long\* counts2\);", header)
    assert "sn_conv_i8z_round_counts" in _hip.SYMBOLS and callable(_hip.conv_i8z_round_counts)
    lib = _hip.load()                                        # binds every declared symbol: AttributeError if one is missing
    assert hasattr(lib, "sn_conv_i8z_round_counts")
    got = _child("""
        lib.sn_conv_i8z_round_counts.argtypes = [ctypes.c_void_p]
        rc = lib.sn_conv_i8z_round_counts(None)
        print(json.dumps([rc, lib.sn_last_error().decode()]))""")
    assert got[0] == -1 and "null pointer" in got[1]         # SN_ERR_INVALID_ARG, before any device call


# --------------------------------------------------------------------------------------------------- the window rule
def _grid(shape, *voxels):
    occ = np.zeros(shape, dtype=bool)
    for v in voxels:
        occ[v] = True
    return occ


def test_rule_on_an_empty_and_a_full_grid():
    assert rule.counts(_grid((1, 12, 8, 64)), 1) == (0, 96)
    assert rule.counts(_grid((1, 12, 8, 64)), 2) == (0, 48)
    assert rule.counts(_grid((2, 20, 20, 48)), 1) == (0, 2 * 20 * 20)
    assert rule.counts(_grid((2, 20, 20, 48)), 2) == (0, 2 * 20 * 10)       # columns of 8, 8 and 4 rows: 4 + 4 + 2 rounds
    assert rule.counts(_grid((1, 7, 5, 16)), 2) == (0, 7 * 3)               # 5 rows: rounds (0, 1) (2, 3) (4)
    assert rule.counts(np.ones((1, 12, 8, 64), bool), 1) == (96, 0)
    assert rule.counts(_grid((1, 64, 64, 128)), 1) == (0, 64 * 64 * 2)      # two y tiles: every (z, x) row twice


def test_rule_one_interior_voxel_is_81_rounds():
    occ = _grid((1, 20, 24, 64), (0, 10, 11, 30))
    assert rule.counts(occ, 1) == (81, 20 * 24 - 81)
    assert rule.counts_exact(occ, 1) == rule.counts(occ, 1)
    # rounds of two rows: rows 7 .. 15 touch the pairs (6, 7) .. (14, 15) = 5 pairs, 9 planes
    assert rule.counts(occ, 2)[0] == 45
    occ = _grid((1, 20, 24, 64), (0, 10, 12, 30))                           # rows 8 .. 16: pairs (8, 9) .. (16, 17)
    assert rule.counts(occ, 2)[0] == 45
    occ = _grid((1, 20, 24, 64), (0, 10, 12, 30), (0, 10, 12, 31))          # a second voxel in the same row changes nothing
    assert rule.counts(occ, 1)[0] == 81


def test_rule_clips_at_faces_and_corners():
    assert rule.counts(_grid((1, 12, 8, 64), (0, 0, 0, 0)), 1)[0] == 5 * 5          # z 0 .. 4, x 0 .. 4
    assert rule.counts(_grid((1, 12, 8, 64), (0, 11, 7, 63)), 1)[0] == 5 * 5
    assert rule.counts(_grid((1, 12, 8, 64), (0, 6, 0, 10)), 1)[0] == 9 * 5
    assert rule.counts(_grid((1, 12, 8, 64), (0, 6, 4, 10)), 1)[0] == 9 * 8         # x 0 .. 8 clipped to the 8 rows
    # the batch index separates tiles
    occ = _grid((2, 12, 8, 64), (1, 0, 0, 0))
    assert rule.counts(occ, 1) == (25, 2 * 96 - 25)


def test_rule_distance_4_is_inside_and_5_is_outside():
    shape = (1, 24, 24, 64)
    for dz, dx, inside in ((4, 0, True), (5, 0, False), (0, 4, True), (0, 5, False), (-4, 0, True), (-5, 0, False),
                           (0, -4, True), (0, -5, False), (4, 4, True), (4, 5, False)):
        occ = _grid(shape, (0, 10 + dz, 12 + dx, 17))
        # the probed output row (z, x) = (10, 12) alone: count with and without a grid cut down to that row's column
        zwin = np.zeros(shape[1:3], bool)
        for z in range(24):
            for xx in range(24):
                zwin[z, xx] = abs(z - (10 + dz)) <= 4 and abs(xx - (12 + dx)) <= 4
        assert zwin[10, 12] == inside
        assert rule.counts(occ, 1)[0] == int(zwin.sum())


def test_rule_sees_the_y_halo_of_the_neighbouring_tile():
    """two y tiles: a voxel at y = 64 .. 67 lies in tile 0's halo (its outputs y = 60 .. 63 need it), one at y = 68 does not;
    a voxel at y = 60 .. 63 lies in tile 1's halo"""
    shape = (1, 12, 8, 128)
    one_tile = 9 * 8
    assert rule.counts(_grid(shape, (0, 6, 4, 30)), 1)[0] == one_tile
    assert rule.counts(_grid(shape, (0, 6, 4, 67)), 1)[0] == 2 * one_tile
    assert rule.counts(_grid(shape, (0, 6, 4, 68)), 1)[0] == one_tile
    assert rule.counts(_grid(shape, (0, 6, 4, 60)), 1)[0] == 2 * one_tile
    assert rule.counts(_grid(shape, (0, 6, 4, 59)), 1)[0] == one_tile
    for y in (30, 59, 60, 67, 68):
        occ = _grid(shape, (0, 6, 4, y))
        assert rule.counts_exact(occ, 1)[0] <= rule.counts(occ, 1)[0]


def test_rule_first_and_second_round_of_a_ticket():
    """variant 2's tickets hold x-rows (2 k, 2 k + 1): a voxel at x = 0 reaches rows 0 .. 4 (of ticket (4, 5) only row 4), a
    voxel at x = 13 reaches rows 9 .. 17 (of ticket (8, 9) only row 9)"""
    shape = (1, 12, 24, 64)
    for xx, rows in ((0, range(0, 5)), (13, range(9, 18))):
        occ = _grid(shape, (0, 6, xx, 40))
        assert rule.counts(occ, 1)[0] == 9 * len(rows)
