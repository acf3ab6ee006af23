"""sn_forward_auto's argument checks and the tables of forward_auto_cases.py, without a GPU.

Every refusal is made before anything is launched: the entry writes the caller's occ_ws, flag and out from its first kernel
on, so an error that comes back after that comes back with side effects.  Without a device a launch cannot succeed, so
SN_ERR_INVALID_ARG / SN_ERR_UNSUPPORTED here (and never SN_ERR_LAUNCH) also says that nothing was tried."""
import ctypes

import numpy as np
import pytest
import torch

from scene_net_amd import _hip

import forward_auto_cases as fc


def _auto(lib, **kw):
    a = dict(x=None, x_dtype=_hip.SN_F32, bank=None, lambdas=None, B=1, Z=4, X=4, Y=8, G=2, kz=3, kx=3, ky=3, occ_ws=None,
             not_binary=None, out=None, out_dtype=_hip.SN_F32)
    a.update(kw)
    return lib.sn_forward_auto(a["x"], a["x_dtype"], a["bank"], a["lambdas"], a["B"], a["Z"], a["X"], a["Y"], a["G"], a["kz"],
                               a["kx"], a["ky"], a["occ_ws"], a["not_binary"], a["out"], a["out_dtype"], None)


def test_argument_checks_need_no_gpu():
    lib = _hip.load()
    buf = ctypes.create_string_buffer(512)
    base = (ctypes.addressof(buf) + 15) // 16 * 16
    p = ctypes.c_void_p(base)
    off = lambda d: ctypes.c_void_p(base + d)   # noqa: E731
    ptrs = dict(x=p, bank=p, lambdas=p, occ_ws=p, not_binary=p, out=p)

    def auto(**kw):
        return _auto(lib, **{**ptrs, **kw})

    def last():
        return lib.sn_last_error()

    for name in ptrs:
        assert auto(**{name: None}) == -1, name
        assert b"null" in last() and (" " + name).encode() in last(), (name, last())
    for name in ("B", "Z", "X", "Y", "G", "kz", "kx", "ky"):
        for v in (0, -1, -(2 ** 31)):
            assert auto(**{name: v}) == -1, (name, v)
            assert b"non-positive" in last() and f" {name} = {v}".encode() in last(), (name, v, last())
    for dt in (_hip.SN_U8, _hip.SN_OCC8, _hip.SN_BF16, _hip.SN_I32, -1, 6):
        assert auto(x_dtype=dt) == -1, dt
        assert f"x_dtype {dt}".encode() in last(), (dt, last())
    # the output contract is sn_conv_bank's: F32 | F64.  (SN_BF16 used to get as far as the second gated block, with the
    # binarize and the linear kernel already enqueued.)
    for dt in (_hip.SN_BF16, _hip.SN_U8, _hip.SN_OCC8, _hip.SN_I32, -1, 6):
        for xdt in (_hip.SN_F32, _hip.SN_F64):
            assert auto(x_dtype=xdt, out_dtype=dt) == -1, (xdt, dt)
            assert f"out_dtype {dt}".encode() in last(), (dt, last())
    for d in (4, 8, 12, 1):
        assert auto(x=off(d)) == -1, d
        assert b"x must be 16-byte aligned" in last(), last()
    for d in (1, 2, 3):
        assert auto(occ_ws=off(d)) == -1, d
        assert b"occ_ws must be 4-byte aligned" in last(), last()
    # shapes no form serves: the fp32 kernel's ky window (every other form falls back to it) and its grid limit
    assert auto(ky=26) == -2 and b"ky=26" in last(), last()
    assert auto(B=1 << 11, Z=1 << 10, X=1 << 10, Y=1 << 10) == -2 and b"too large" in last(), last()
    # the checks come in the order the message names: a null pointer before a bad extent before a dtype
    assert auto(x=None, B=0, out_dtype=_hip.SN_BF16) == -1 and b"null pointer x" in last()
    assert auto(B=0, out_dtype=_hip.SN_BF16) == -1 and b"extent B" in last()


def test_wrapper_refuses_the_same_before_any_device_work():
    x = torch.zeros((1, 1, 4, 4, 8))
    bank, lam = torch.zeros((2, 3, 3, 3)), torch.zeros(2)
    for dt in (torch.bfloat16, torch.uint8, torch.bool, torch.float16, torch.int32):
        with pytest.raises(_hip.HipLibraryError, match="out_dtype"):
            _hip.forward_auto(x, bank, lam, out_dtype=dt)
    for dt in (torch.uint8, torch.bool, torch.bfloat16, torch.int32):
        with pytest.raises(_hip.HipLibraryError, match="x dtype"):
            _hip.forward_auto(x.to(dt), bank, lam)
    with pytest.raises(_hip.HipLibraryError, match=r"\[B,1,Z,X,Y\]"):
        _hip.forward_auto(x[0], bank, lam)
    with pytest.raises(_hip.HipLibraryError, match="no CPU path"):
        _hip.forward_auto(x, bank, lam)


@pytest.mark.parametrize("np_dtype", [np.float32, np.float64])
def test_value_table_in_numpy(np_dtype):
    """what the issue states of the reference: occ 0 for the two zeros and 1 for every other entry; only +-0 and 1.0 keep the
    flag down -- a subnormal is nonzero and raises it"""
    table = fc.odd_values(np_dtype)
    assert len(table) == 13 and len({n for n, _ in table}) == 13
    for name, v in table:
        assert v.dtype == np_dtype
        occ, flag = fc.np_binarize(np.array([v]))
        assert occ[0] == (0 if name in ("+0", "-0") else 1), name
        assert flag == (0 if name in ("+0", "-0", "1") else 1), name
    assert np.signbit(dict(table)["-0"]) and dict(table)["subnormal"] > 0
    occ, flag = fc.np_binarize(fc.binary_grid((3, 5, 7), 0.2, 1).astype(np_dtype))
    assert flag == 0 and 0 < occ.sum() < occ.size


def test_positions_cover_every_class_of_the_launch_geometry():
    pos = fc.positions()
    for q in pos + fc.big_positions():
        assert 0 <= q.index < int(np.prod(q.shape)) and len(q.shape) == 5 and q.shape[1] == 1, q
    tails = {}
    for q in pos:
        n = int(np.prod(q.shape))
        if q.index >= n // 4 * 4 and n >= 4:
            tails.setdefault(n % 4, set()).add(q.index - n // 4 * 4)
    assert tails == {1: {0}, 2: {0, 1}, 3: {0, 1, 2}}
    assert {int(np.prod(q.shape)) for q in pos} >= {1, 2, 3}
    n = 1399
    assert any(q.index == n // 4 * 4 - 1 and int(np.prod(q.shape)) == n for q in pos)
    assert any(q.index == 0 for q in pos)
    body = [q for q in pos if int(np.prod(q.shape)) == n and q.index < n // 4 * 4]
    assert any((q.index // 4) % 64 != 0 and (q.index // 4) % 256 >= 64 for q in body)        # a lane and a wave other than 0
    assert any(q.index // 4 >= 256 for q in body)                                             # a block other than 0
    # one trip serves STRIDE_ELEMENTS elements, and only with all 2048 blocks launched is there a second one
    nb = int(np.prod(fc.BIG))
    assert min((nb // 4 + 255) // 256 + 1, 2048) == 2048 and fc.STRIDE_ELEMENTS == 2_097_152
    assert sum(q.index >= fc.STRIDE_ELEMENTS for q in fc.big_positions()) >= 3


def test_routes_are_the_ones_the_plan_queries_name():
    """no shape is taken on trust: the table's routes against sn_conv_fused_supported / _plan and sn_conv_bank_plan (host
    only, 256 compute units assumed without a device; none of these answers depends on the count)"""
    for name, r in fc.ROUTES.items():
        assert fc.route_plan(name) == (r.fused, r.bool_kernel, r.w24), (name, fc.route_plan(name))
        assert _hip.conv_bank_plan((torch.float32, r.shape), (r.G,) + r.ks).kernel == "fp32"
        assert (r.shape[4] % 4 != 0) == (r.bool_kernel == "fp32"), name
    xb = torch.zeros((1, 1, 9, 9, 64), dtype=torch.bool)
    answers = {ks: _hip.conv_fused_supported(xb, ks) for ks in fc.STRIDE4_QUERIES}
    print("conv_fused_supported on (1,1,9,9,64):", answers)
    assert answers == fc.STRIDE4_QUERIES
    assert set(fc.DECLINED_ROUTES + fc.NONBINARY_ROUTES + fc.BINARY_ROUTES) == set(fc.ROUTES)
