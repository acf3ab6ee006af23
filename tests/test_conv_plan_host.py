"""sn_conv_bank_plan (include/scenenet_hip.h) on the host: what sn_conv_bank would launch, asked without a device.

The four hand-written kernels behind sn_conv_bank (csrc/conv_fp32.inc, conv_i8.hip, conv_i8s.hip and its folded form) pick
their workgroup tile from one ladder, {8,8} {4,8} {4,4} {2,4} {1,4} {1,2} (TZ, TX; TY = 64): the first rung that fits LDS
and gives at least 4 tiles per compute unit, else the last one that fits.  Without a device the ladder counts 256 compute
units, so the threshold is 1024 tiles; every pin below is that arithmetic done by hand on the code, none was read off the
query.  The queries run in one child process that hides every device, so the pins hold on a machine that has one."""
import json
import os
import subprocess
import sys

import pytest

from scene_net_amd import _hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

C2 = (32, 64, 64, 64)            # BASELINE C2's batch
RAGGED = (61, 59, 132)           # nothing a multiple of a tile; three y tiles, the last 4 columns wide
# B, (Z, X, Y), rung: the first rung with >= 1024 tiles (tiles of a rung: B * ceil(Z / TZ) * ceil(X / TX) * 3)
RUNG_TABLE = [
    (6, (61, 59, 132), (8, 8)),      # 6 * 8 * 8 * 3 = 1152
    (3, (61, 59, 132), (4, 8)),      # 8x8: 576;  4x8: 3 * 16 * 8 * 3 = 1152
    (2, (61, 59, 132), (4, 4)),      # 384; 768;  4x4: 2 * 16 * 15 * 3 = 1440
    (1, (61, 59, 132), (2, 4)),      # 4x4: 720;  2x4: 31 * 15 * 3 = 1395
    (1, (30, 59, 132), (1, 4)),      # 2x4: 675;  1x4: 30 * 15 * 3 = 1350
    (256, (5, 13, 68), (8, 8)),      # 256 * 1 * 2 * 2 = 1024: a grid smaller than the tile in z
]
RUNG_TILES = {0: 1152, 1: 1152, 2: 1440, 3: 1395, 4: 1350, 5: 1024}
FP32, OCC = "float32", "bool"


def _queries():
    """name -> (dtype, (B, Z, X, Y), (G, kz, kx, ky), options)"""
    q = {
        "c2_fp32": (FP32, C2, (16, 9, 9, 9), {}),
        "c2_occ": (OCC, C2, (16, 9, 9, 9), {}),
        "c2_nofold": (OCC, C2, (16, 9, 9, 9), {"conv_i8_fold": 0}),
        "c2_legacy": (OCC, C2, (16, 9, 9, 9), {"conv_i8_legacy": 1}),
        "c2_legacy_nostage": (OCC, C2, (16, 9, 9, 9), {"conv_i8_legacy": 1, "conv_i8_no_stage": 1}),
        "c2_no_i8": (OCC, C2, (16, 9, 9, 9), {"conv_no_i8": 1}),
        "c2_skip_empty": (OCC, C2, (16, 9, 9, 9), {"conv_skip_empty_tiles": 1}),
        "ref_default_bank": (OCC, (64, 64, 64, 64), (3, 9, 5, 5), {}),
        "wide_rows": (OCC, (64, 64, 64, 64), (2, 3, 3, 17), {}),
        "two_groups": (OCC, C2, (20, 9, 9, 9), {}),
        "two_groups_fp32": (FP32, C2, (20, 9, 9, 9), {}),
        "y_not_16": (OCC, (6,) + RAGGED, (16, 9, 9, 9), {}),
        "y_not_4": (OCC, (6, 61, 59, 130), (16, 9, 9, 9), {}),
    }
    for i, (B, grid, _) in enumerate(RUNG_TABLE):
        q[f"rung{i}_fp32"] = (FP32, (B,) + grid, (16, 9, 9, 9), {})
        q[f"rung{i}_f64"] = ("float64", (B,) + grid, (5, 9, 7, 7), {})
        q[f"rung{i}_four_copy"] = (OCC, (B,) + grid, (16, 9, 9, 9), {"conv_i8_legacy": 1, "conv_i8_no_stage": 1})
        q[f"rung{i}_four_copy_955"] = (OCC, (B,) + grid, (3, 9, 5, 5), {"conv_i8_no_stage": 1})
        # the stride-4 kernel wants Y % 16 == 0: 144 and 80 have the y tiles of 132 and 68
        grid16 = grid[:2] + ({132: 144, 68: 80}[grid[2]],)
        q[f"rung{i}_stride4"] = (OCC, (B,) + grid16, (16, 9, 9, 9), {"conv_i8_fold": 0})
        q[f"rung{i}_folded"] = (OCC, (B,) + grid16, (16, 9, 9, 9), {})
    n = 0
    for B in (1, 2, 3, 6, 32, 256):
        for grid in (RAGGED, (30, 59, 132), (5, 13, 68), (64, 64, 64), (8, 8, 64)):
            q[f"dbl{n}"] = (FP32, (B,) + grid, (16, 9, 9, 9), {"conv_double_buffer": 1})
            n += 1
    return q


_CHILD = """
import json, sys
sys.path.insert(0, sys.argv[1])
import torch
from scene_net_amd import _hip
out = {}
for name, (dtype, grid, bank, opts) in json.loads(sys.argv[2]).items():
    B, Z, X, Y = grid
    with _hip.options(**opts):
        out[name] = _hip.conv_bank_plan((getattr(torch, dtype), (B, 1, Z, X, Y)), bank)._asdict()
print(json.dumps(out))
"""


@pytest.fixture(scope="module")
def plans():
    env = {k: v for k, v in os.environ.items() if not k.startswith("SN_")}
    env.update(HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")   # no device: the ladder counts 256 compute units
    p = subprocess.run([sys.executable, "-c", _CHILD, ROOT, json.dumps(_queries())], env=env, capture_output=True,
                       text=True, timeout=600)
    assert p.returncode == 0, p.stderr
    got = json.loads(p.stdout.strip().splitlines()[-1])
    assert all(v["cus"] == 256 for v in got.values())
    return got


def _is(plan, kernel, rung, **more):
    assert (plan["kernel"], (plan["tz"], plan["tx"])) == (kernel, rung), plan
    for k, v in more.items():
        assert plan[k] == v, (k, plan)


def test_c2_batch_plans_the_big_tile(plans):
    _is(plans["c2_fp32"], "fp32", (8, 8), ntiles=2048, double_buffered=False, staged=False, row_stride=352)
    # the host's half of the folded / stride-4 choice: same ladder (plan_stride4), same tiles
    _is(plans["c2_occ"], "folded", (8, 8), ntiles=2048, row_stride=96)
    _is(plans["c2_nofold"], "stride4", (8, 8), ntiles=2048, row_stride=96)


def test_c2_four_copy_staged_and_unstaged(plans):
    _is(plans["c2_legacy"], "four_copy", (8, 8), ntiles=2048, staged=True, row_stride=80)
    _is(plans["c2_legacy_nostage"], "four_copy", (8, 8), ntiles=2048, staged=False, row_stride=96)
    # tile skipping lives in the four-copy kernel; conv_no_i8 is the fp32 kernel on the same bytes
    _is(plans["c2_skip_empty"], "four_copy", (8, 8), staged=True)
    _is(plans["c2_no_i8"], "fp32", (8, 8), ntiles=2048)


def test_kernel_sizes_only_the_four_copy_kernel_serves(plans):
    """ky != 9: the reference's own default bank (9,5,5) runs the staged template at the big tile; ky = 17 needs more than
    80 bytes of a halo row (need = delta + 15 + 48 + 4 C + 3 = 0 + 66 + 20 = 86), so it is unstaged at every tile."""
    _is(plans["ref_default_bank"], "four_copy", (8, 8), ntiles=4096, staged=True, row_stride=80)
    _is(plans["wide_rows"], "four_copy", (8, 8), ntiles=4096, staged=False, row_stride=96)


def test_more_than_16_kernels_reports_the_first_group(plans):
    assert plans["two_groups"] == plans["c2_occ"]
    assert plans["two_groups_fp32"] == plans["c2_fp32"]


def test_y_alignment_picks_the_kernel(plans):
    """Y % 16 != 0: not the stride-4 kernel; Y % 4 != 0: no int8 kernel at all"""
    _is(plans["y_not_16"], "four_copy", (8, 8), ntiles=1152, staged=True)
    _is(plans["y_not_4"], "fp32", (8, 8), ntiles=1152)


@pytest.mark.parametrize("i", range(len(RUNG_TABLE)))
def test_ragged_rung_table(plans, i):
    rung = RUNG_TABLE[i][2]
    _is(plans[f"rung{i}_fp32"], "fp32", rung, ntiles=RUNG_TILES[i], double_buffered=False)
    _is(plans[f"rung{i}_f64"], "fp32", rung, ntiles=RUNG_TILES[i])
    _is(plans[f"rung{i}_four_copy"], "four_copy", rung, ntiles=RUNG_TILES[i], staged=False, row_stride=96)
    _is(plans[f"rung{i}_four_copy_955"], "four_copy", rung, ntiles=RUNG_TILES[i], staged=False)
    _is(plans[f"rung{i}_stride4"], "stride4", rung, ntiles=RUNG_TILES[i])
    _is(plans[f"rung{i}_folded"], "folded", rung, ntiles=RUNG_TILES[i])


def test_double_buffer_at_9_cubed_stays_within_its_staging_registers(plans):
    """a wave stages 18 halo rows in registers: (TZ + 8)(TX + 8) <= 8 * 18 = 144, so {4,4} is the largest tile at 9^3"""
    seen = set()
    for name, p in plans.items():
        if name.startswith("dbl"):
            assert p["kernel"] == "fp32" and p["double_buffered"], p
            assert (p["tz"] + 8) * (p["tx"] + 8) <= 144, p
            seen.add((p["tz"], p["tx"]))
    assert (4, 4) in seen and (8, 8) not in seen and (4, 8) not in seen


def test_argument_checks():
    lib = _hip.load()
    import ctypes
    p8 = (ctypes.c_int32 * 8)()
    p = ctypes.cast(p8, ctypes.c_void_p)
    assert lib.sn_conv_bank_plan(0, 1, 8, 8, 64, 4, 3, 3, 3, None) == -1
    assert lib.sn_conv_bank_plan(0, 0, 8, 8, 64, 4, 3, 3, 3, p) == -1
    assert lib.sn_conv_bank_plan(7, 1, 8, 8, 64, 4, 3, 3, 3, p) == -1
    assert b"x_dtype" in lib.sn_last_error()
    assert lib.sn_conv_bank_plan(0, 1, 8, 8, 70, 4, 3, 3, 26, p) == -2     # where sn_conv_bank refuses: ky > 25
    assert lib.sn_conv_bank_plan(0, 1, 8, 8, 64, 4, 3, 3, 3, p) == 0 and list(p8)[:3] == [0, 1, 2] and p8[7] == 0
    with pytest.raises(_hip.HipLibraryError):
        _hip.conv_bank_plan((__import__("torch").float32, (1, 2, 8, 8, 64)), (4, 3, 3, 3))
