"""The CPU model of K3L's pre-activation (tests/lin_cases.py: model_pre) against the fp64 oracle, on any machine.

test_gpu_conv_lin_walk.py holds the kernel to that model at 3 x 2^-23; here the model itself is held to
oracle.geneo_oracle.conv_bank, elementwise, at every kernel size of the table on a B = 3 batch of the ragged grid:

    |pre_model - pre_ref| <= quant_bound(K*) + 2^-22 |pre_ref|

quant_bound (test_gpu_conv_i8_envelope.py) is the worst case over binary inputs of the 24-bit fixed point -- what the
kernel's own guard computes --, and 2^-22 = 4 x 2^-24 covers the model's four fp32 roundings: f32(low), the fma, the scale
and the product.  [measured, CPU] the largest ratio to this bar over the table is 0.45.

Also here: the digits recombine to Q, the chain is exact (asserted inside the model), the guard keeps every case on K3L, and
the plan query (sn_conv_fused_plan: host arithmetic, no device) puts every size of the table on the fork it is there for."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from scene_net_amd import _hip

import lin_cases as lc
from test_gpu_conv_i8_envelope import quant_bound

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B_HOST = 3
ELEMENTS = (0, 1, 2)      # 0.3, full, empty


@pytest.mark.parametrize("name", list(lc.SIZES))
def test_model_against_the_fp64_oracle(name):
    size = lc.SIZES[name]
    got = lc.checked(name, "ragged", B_HOST, ELEMENTS)      # (asserts the exact chain, both signs, 0.5 <= max|pre| <= 3)
    t = got.tables
    # the digits: balanced, and they recombine to Q, which spans the 24 bits
    d0, d1, d2 = t.digits
    assert np.array_equal(d0 + 256 * d1 + 65536 * d2, t.Q)
    assert np.abs(d0).max() <= 128 and np.abs(d1).max() <= 128 and np.abs(d2).max() <= 128
    assert np.abs(t.Q).max() == 8355711
    assert got.low_max < 2 ** 31
    # the guard will keep the launch on K3L
    bound = quant_bound(t.kstar)
    assert bound < 0.5 * 9e-5, (name, bound)
    assert 1e-9 * _hip.get_option("conv_i8_tolerance_ppb") == pytest.approx(9e-5)
    # the model, elementwise
    pre, ref = got.pre.astype(np.float64), got.ref
    bar = bound + 2.0 ** -22 * np.abs(ref)
    err = np.abs(pre - ref)
    ratio = float((err / (bar + 1e-300)).max())
    print(f"{name} G={size.G}: max|pre| {np.abs(ref[0]).max():.3f} (full element {np.abs(ref[1]).max():.3f}), "
          f"quant bound {bound:.2e}, max err {err.max():.2e}, worst ratio to the bar {ratio:.3f}")
    assert (err <= bar).all(), (name, ratio)
    assert not pre[2].any() and not ref[2].any()              # the empty element


_CHILD = """
import json, sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import lin_cases as lc
out = {}
for name, size in lc.SIZES.items():
    for gname in (("ragged", "thin") if size.thin else ("ragged",)):
        grid = lc.GRIDS[gname]
        B, p = lc.walk_batch(size, grid)
        out[f"{name}-{gname}"] = dict(B=B, plan=p._asdict(), one=lc.plan_of(size, 1, grid)._asdict())
print(json.dumps(out))
"""


@pytest.fixture(scope="module")
def plans():
    """every case's batch size and plans, from a child process that hides every device: 256 compute units are counted"""
    env = {k: v for k, v in os.environ.items() if not k.startswith("SN_")}
    env.update(HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    p = subprocess.run([sys.executable, "-c", _CHILD, ROOT], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr
    return json.loads(p.stdout.strip().splitlines()[-1])


def test_every_size_is_on_its_fork_and_walks_at_256_compute_units(plans):
    assert set(plans) == {f"{n}-{g}" for n, g in lc.WALK_CASES}
    for key, row in plans.items():
        name, gname = key.rsplit("-", 1)
        plan, one = _hip.ConvFusedPlan(**row["plan"]), _hip.ConvFusedPlan(**row["one"])
        per_element = {"ragged": 18, "thin": 3}[gname]
        assert row["B"] == {"ragged": 36, "thin": 214}[gname], (key, row["B"])
        assert (plan.cus, plan.workgroups, plan.ntiles) == (256, 256, row["B"] * per_element), (key, plan)
        assert (plan.tiles_per_workgroup_min, plan.tiles_per_workgroup_max) == (2, 3), (key, plan)
        assert not lc.plan_misses(plan, lc.SIZES[name].plan), (key, lc.plan_misses(plan, lc.SIZES[name].plan))
        assert plan.lds_bytes <= 160 * 1024
        # an element alone: one tile per workgroup, the same fork
        assert (one.ntiles, one.workgroups) == (per_element, per_element), (key, one)
        assert one.tiles_per_workgroup_max == 1 and not lc.plan_misses(one, lc.SIZES[name].plan), (key, one)


def test_every_fork_of_the_coverage_table_is_reachable(plans):
    for fork, hit in lc.FORKS.items():
        names = [k for k, row in plans.items() if hit(_hip.ConvFusedPlan(**row["plan"]), lc.SIZES[k.rsplit("-", 1)[0]].ks)]
        print(f"{fork}: {names}")
        assert names, fork


def test_plan_is_refused_like_the_launch():
    lib = _hip.load()
    p8 = (ctypes.c_int32 * 8)()
    p = ctypes.cast(p8, ctypes.c_void_p)
    assert lib.sn_conv_fused_plan(1, 8, 8, 64, 1, 3, 3, 18, p) == -2        # ky = 18: a strip's window leaves 32 bytes
    assert lib.sn_conv_fused_plan(1, 8, 8, 64, 1, 13, 13, 9, p) == -2       # tables + halo over 160 KiB
    assert lib.sn_conv_fused_supported(1, 8, 8, 64, 13, 13, 9) == 0 and lib.sn_conv_fused_supported(1, 8, 8, 64, 3, 3, 18) == 0
    assert lib.sn_conv_fused_plan(1, 8, 8, 64, 1, 9, 9, 9, p) == 0
    assert list(p8)[:5] == [1, 31, 1, 16, 1] and p8[5] == 1                  # one tile, one workgroup
    with _hip.options(conv_lin_no24=1):
        assert lib.sn_conv_fused_plan(1, 8, 8, 64, 1, 9, 9, 9, p) == 0 and list(p8)[:3] == [0, 41, 1]
        # 99 kernel rows at 32 bytes: 50 steps, tables of 153 KiB + the halo over the LDS -- these sizes have the 24-byte form only
        for name, size in lc.SIZES.items():
            want = 0 if size.ks[0] * size.ks[1] < 99 else -2
            assert lib.sn_conv_fused_plan(1, 8, 8, 64, 1, *size.ks, p) == want, name
    with pytest.raises(_hip.HipLibraryError):
        _hip.conv_fused_plan((1, 2, 8, 8, 64), (3, 3, 3))
    assert _hip.conv_fused_plan((2, 1, 8, 16, 128), (3, 3, 3)).ntiles == 4
