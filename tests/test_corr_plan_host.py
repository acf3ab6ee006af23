"""sn_conv_corr_plan (include/scenenet_hip.h) on the host: what sn_conv_corr_ws would launch, asked without a device.

The query runs the planners the launches run (csrc/corr.hip plan / plan_sparse, csrc/backward.hip tap_plan), under the
options in force.  Pinned here: its agreement with sn_conv_corr_blocks / sn_conv_corr_ws_bytes, the routing rules
(corr_dense, non-binary input, kernel extents past 16, bf16 gradients), the training shape's job counts, and -- the table
of corr_plan_cases.py -- that every shape of tests/test_gpu_corr_plans.py still lands on the fork it is there for."""
import ctypes

import pytest
import torch

from scene_net_amd import _hip

import corr_plan_cases as cases

DT = {"bool": torch.bool, "uint8": torch.uint8, "float32": torch.float32, "float64": torch.float64,
      "bfloat16": torch.bfloat16}
ROWS = cases.all_cases()


def _plan(x_dtype, shape, ks, opts, g_dtype=torch.float32):
    with _hip.options(**opts):
        return _hip.conv_corr_plan((x_dtype, shape), ks, g_dtype)


def _raw(x_dtype, g_dtype, B, Z, X, Y, kz, kx, ky, p=True):
    p8 = (ctypes.c_int32 * 8)()
    rc = _hip.load().sn_conv_corr_plan(x_dtype, g_dtype, B, Z, X, Y, kz, kx, ky,
                                       ctypes.cast(p8, ctypes.c_void_p) if p else None)
    return rc, list(p8)


@pytest.mark.parametrize("name", sorted(ROWS))
def test_gpu_test_shapes_reach_their_forks(name):
    x, g, case = ROWS[name]
    plan = _plan(DT[x], case.shape, case.ks, case.opts, DT[g])
    assert not cases.fork_misses(plan, case.fork), (name, plan)


@pytest.mark.parametrize("name", sorted(ROWS))
def test_plan_agrees_with_blocks_and_workspace(name):
    """workgroups (= partial rows written) <= sn_conv_corr_blocks; the workspace holds them; 1 <= workgroups <= jobs; the LDS
    tile is within what a workgroup may ask for"""
    lib = _hip.load()
    x, g, case = ROWS[name]
    B, _, Z, X, Y = case.shape
    taps = case.ks[0] * case.ks[1] * case.ks[2]
    with _hip.options(**case.opts):
        plan = _hip.conv_corr_plan((DT[x], case.shape), case.ks, DT[g])
        ws = int(lib.sn_conv_corr_ws_bytes(_hip._DT[DT[x]], B, Z, X, Y, *case.ks))
    blocks = int(lib.sn_conv_corr_blocks(B, Z, X, Y))
    assert 1 <= plan.workgroups <= plan.jobs and plan.workgroups <= blocks, plan
    assert ws >= blocks * taps * 4 >= plan.workgroups * taps * 4
    assert 0 < plan.lds_bytes <= 160 * 1024
    assert plan.row_tiles == -(-X // plan.rows)
    if plan.kernel != "taps":
        assert plan.jobs == B * Z * plan.row_tiles and plan.workgroups <= 768
        assert plan.kzmax == (9 if case.ks[0] <= 9 else 16)
    else:
        assert plan.jobs == plan.workgroups == B * -(-Z // 8) * -(-X // 8) * -(-Y // 64) and plan.kzmax == 0


def test_training_shape_job_counts():
    """32 x 64^3 with the 9^3 kernel: 4096 gather jobs / 2048 GEMM jobs on 768 persistent workgroups; the largest shape the
    older tests compare with a reference (4 x 64^3) gives every workgroup exactly one job"""
    c2 = (32, 1, 64, 64, 64)
    k4s = _plan(torch.bool, c2, (9, 9, 9), cases.gather(0))
    assert (k4s.kernel, k4s.jobs, k4s.workgroups, k4s.rows, k4s.row_tiles, k4s.kzmax) == ("gather", 4096, 768, 32, 2, 9)
    assert k4s.vec and k4s.list_vec and k4s.multi_group
    k4 = _plan(torch.bool, c2, (9, 9, 9), cases.DENSE)
    assert (k4.kernel, k4.jobs, k4.workgroups, k4.rows, k4.row_tiles, k4.kzmax) == ("gemm", 2048, 768, 64, 1, 9)
    assert k4.vec and not k4.every_step
    small = (4, 1, 64, 64, 64)
    assert _plan(torch.bool, small, (9, 9, 9), cases.gather(0))[3:5] == (512, 512)
    assert _plan(torch.bool, small, (9, 9, 9), cases.DENSE)[3:5] == (256, 256)


@pytest.mark.parametrize("shape,ks", [((4, 1, 64, 64, 64), (9, 9, 9)), ((2, 1, 12, 10, 20), (5, 5, 5)),
                                      ((1, 1, 5, 12, 16), (3, 17, 17)), ((1, 1, 4, 6, 300), (3, 5, 17)),
                                      ((1, 1, 3, 9, 1700), (3, 3, 3))])
def test_only_binary_input_without_corr_dense_gathers(shape, ks):
    for dt in (torch.float32, torch.float64, torch.uint8):
        for opts in (cases.gather(0), cases.gather(64), cases.DENSE):
            assert _plan(dt, shape, ks, opts).kernel != "gather"
    assert _plan(torch.bool, shape, ks, cases.DENSE).kernel != "gather"
    # and the query follows the workspace: no list room asked for <=> no gather planned
    lib = _hip.load()
    B, _, Z, X, Y = shape
    taps = ks[0] * ks[1] * ks[2]
    rows_only = int(lib.sn_conv_corr_blocks(B, Z, X, Y)) * taps * 4
    with _hip.options(**cases.gather(0)):
        ws = int(lib.sn_conv_corr_ws_bytes(_hip.SN_OCC8, B, Z, X, Y, *ks))
        gathers = _hip.conv_corr_plan((torch.bool, shape), ks).kernel == "gather"
    assert ws >= rows_only and (not gathers or ws > 0)
    if ws > rows_only:
        assert gathers


def test_extent_17_takes_the_fallback_and_refuses_bf16():
    shape = (1, 1, 4, 6, 300)
    for ks in ((3, 5, 17), (3, 17, 5), (17, 3, 3)):
        for dt in (torch.float32, torch.bool):
            p = _plan(dt, shape, ks, cases.DENSE)
            assert p.kernel == "taps" and p.kzmax == 0 and not (p.vec or p.list_vec or p.every_step or p.multi_group)
            with pytest.raises(_hip.HipLibraryError, match="bf16 gradients"):
                _plan(dt, shape, ks, cases.DENSE, torch.bfloat16)
    # the gather has no such limit in x and y: binary input keeps its bf16 gradients at ky = 17
    assert _plan(torch.bool, shape, (3, 5, 17), cases.gather(0), torch.bfloat16).kernel == "gather"


def test_flag_bits():
    """bit 0 / 1: Y % 4 / Y % 8 (gather: the delta tile within 4096 elements too); bit 2: more than 32 K steps (Y > 128);
    bit 3: 512 // (kx ky) > 1"""
    for Y, vec, list_vec in ((16, True, True), (12, True, False), (13, False, False), (130, False, False)):
        p = _plan(torch.bool, (1, 1, 4, 6, Y), (3, 3, 3), cases.gather(0))
        assert (p.kernel, p.vec, p.list_vec) == ("gather", vec, list_vec), (Y, p)
        d = _plan(torch.bool, (1, 1, 4, 6, Y), (3, 3, 3), cases.DENSE)
        assert (d.kernel, d.vec, d.list_vec, d.every_step) == ("gemm", vec, False, Y > 128), (Y, d)
    assert not _plan(torch.bool, (1, 1, 4, 6, 128), (3, 3, 3), cases.DENSE).every_step
    assert _plan(torch.bool, (1, 1, 4, 6, 129), (3, 3, 3), cases.DENSE).every_step
    # the planner keeps a job's delta rows within 3072 elements, so the quads' 4096 never bind: Y % 4 alone decides bit 0
    wide = _plan(torch.bool, (1, 1, 4, 16, 256), (3, 3, 3), cases.gather(0))
    assert wide.kernel == "gather" and (wide.rows + 2) * 256 <= 3072 and wide.vec
    assert _plan(torch.bool, (1, 1, 4, 20, 16), (3, 16, 16), cases.gather(0)).multi_group
    assert not _plan(torch.bool, (1, 1, 4, 20, 16), (3, 16, 17), cases.gather(0)).multi_group


def test_argument_checks():
    rc, _ = _raw(_hip.SN_OCC8, _hip.SN_F32, 1, 8, 8, 16, 3, 3, 3, p=False)
    assert rc == -1 and b"null" in _hip.load().sn_last_error()
    assert _raw(_hip.SN_OCC8, _hip.SN_F32, 0, 8, 8, 16, 3, 3, 3)[0] == -1
    assert _raw(_hip.SN_OCC8, _hip.SN_F32, 1, 8, 8, 16, 3, 0, 3)[0] == -1
    assert _raw(_hip.SN_BF16, _hip.SN_F32, 1, 8, 8, 16, 3, 3, 3)[0] == -1      # bf16 is never an input grid
    assert _raw(_hip.SN_OCC8, _hip.SN_U8, 1, 8, 8, 16, 3, 3, 3)[0] == -1       # gradients are f32 or bf16
    rc, _ = _raw(_hip.SN_F32, _hip.SN_BF16, 1, 8, 8, 16, 3, 3, 17)
    assert rc == -2 and b"sn_conv_corr_plan" in _hip.load().sn_last_error()
    assert _raw(_hip.SN_F32, _hip.SN_F32, 1, 8, 8, 16, 40, 40, 40)[0] == -2    # too large for the thread-per-tap tile
    rc, p8 = _raw(_hip.SN_OCC8, _hip.SN_F32, 1, 8, 8, 16, 3, 3, 3)
    assert rc == 0 and p8[0] == 2 and p8[5] == 9
    with pytest.raises(_hip.HipLibraryError):
        _hip.conv_corr_plan((torch.float32, (1, 2, 8, 8, 16)), (3, 3, 3))
    with pytest.raises(_hip.HipLibraryError):
        _hip.conv_corr_plan((torch.bfloat16, (1, 1, 8, 8, 16)), (3, 3, 3))
