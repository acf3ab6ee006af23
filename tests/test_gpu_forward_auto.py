"""sn_forward_auto (csrc/conv_lin.hip) on the MI355X: the forward every f32 / f64 grid takes through SceneNet.forward.

The entry classifies x on the device (binarize_kernel: (x != 0) bytes and a "not binary" flag), then enqueues the int8 form
and the fp32 form of the same forward, each behind a device-side gate, with the int8 kernels' own quantisation-guard gate
nested inside.  A kernel that ignores its gate, a flag that is not reset, a missed tail element: each still gives a plausible
forward.  So the tests call the C entry with buffers of their own (as test_gpu_backward.py does for sn_conv_corr_ws): occ_ws
pre-filled with 0xAB and followed by guard bytes, the flag with -7, out with NaN.

B. binarize_kernel against numpy, bit for bit, for every value of forward_auto_cases.odd_values at every position class of
   the launch geometry (forward_auto_cases.positions, big_positions).
C. routes.  Which kernels a case runs is asked of the library (conv_fused_supported, conv_fused_plan, conv_bank_plan) and
   held to forward_auto_cases.ROUTES; each case then asserts
     1. out equals, bit for bit, the sibling entry that runs the form the flag and the guard select,
     2. |out - oracle| < 1e-4 everywhere (fp64 oracle; the project's parity bar), and no NaN is left,
     3. the flag is numpy's.
   What tells the forms apart is that they differ in their bits: `other` below is the form that must NOT have written out,
   and `not torch.equal(winner, other)` is asserted first (the bank's kernel scales are taken from
   forward_auto_cases.SPANS until it holds).  There is one kind of case where the two forms cannot differ: a binary x on a
   grid with Y % 4 != 0, where the int8 form IS the fp32 kernel on the bytes and the fp32 form the same kernel on the same
   numbers as floats.  There the case asserts 1 - 3 only (a launch that ran twice or not at all still shows as a NaN left
   or a missed oracle bar), and the non-binary and NaN grids on the same shapes tell the forms apart.
   The stride-4 kernel can be reached from this entry only for ky = 9, kz kx = 81, Y % 16 == 0 where the linear kernel
   declines.  conv_fused_supported on (1,1,9,9,64) answers: (27,3,9) True, (3,27,9) True, (81,1,9) False, (1,81,9) True
   (test_forward_auto_host.py asserts and prints them), so (81,1,9) with G = 3 is a route of its own here.
D. eight calls back to back on one stream, one synchronisation at the end.
E. one captured call replayed while the content of x changes class.
F. the wrapper on a misaligned view, SceneNet.forward in eval and under autograd."""
import functools

import numpy as np
import pytest
import torch

import scene_net_amd as sna
from scene_net_amd import _hip

import forward_auto_cases as fc

pytestmark = pytest.mark.gpu
TOL = fc.TOL
_OUT_CODE = {torch.float32: _hip.SN_F32, torch.float64: _hip.SN_F64, torch.bfloat16: _hip.SN_BF16}


# ------------------------------------------------------------------------------------------------------------- helpers
class Buffers:
    """occ_ws (+ guard bytes), flag and out of one call, poisoned"""

    def __init__(self, shape, out_dtype, dev):
        self.n = int(np.prod(shape))
        self.occ_all = torch.empty(self.n + fc.GUARD_BYTES, dtype=torch.uint8, device=dev)
        self.flag = torch.empty(1, dtype=torch.int32, device=dev)
        self.out = torch.empty(shape, dtype=out_dtype, device=dev)
        self.poison()

    def poison(self):
        self.occ_all.fill_(fc.OCC_POISON)
        self.flag.fill_(fc.FLAG_POISON)
        self.out.fill_(float("nan"))

    @property
    def occ(self):
        return self.occ_all[:self.n]

    def guard_intact(self):
        return bool((self.occ_all[self.n:] == fc.OCC_POISON).all().item())


def _raw(x, bank, lam, buf, out_code=None):
    """the C entry on the current stream; returns its status"""
    B, _, Z, X, Y = x.shape
    G, kz, kx, ky = bank.shape
    assert x.is_contiguous() and bank.is_contiguous() and bank.dtype == torch.float32 and lam.dtype == torch.float32
    return _hip.load().sn_forward_auto(x.data_ptr(), _hip._DT[x.dtype], bank.data_ptr(), lam.data_ptr(), B, Z, X, Y, G, kz,
                                       kx, ky, buf.occ_all.data_ptr(), buf.flag.data_ptr(), buf.out.data_ptr(),
                                       _OUT_CODE[buf.out.dtype] if out_code is None else out_code, _hip._stream())


def _auto(x, bank, lam, out_dtype, buf=None):
    """-> Buffers after one call on poisoned buffers"""
    buf = Buffers(tuple(x.shape), out_dtype, x.device) if buf is None else buf
    rc = _raw(x, bank, lam, buf)
    assert rc == 0, (rc, _hip.load().sn_last_error())
    return buf


def _first_difference(a, b):
    bad = (a != b).nonzero()
    return (len(bad), bad[0].tolist(), a[tuple(bad[0])].item(), b[tuple(bad[0])].item()) if len(bad) else None


def _same_bits(a, b):
    """bit for bit, NaN included"""
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _check_classification(buf, x_host_np, what):
    occ_ref, flag_ref = fc.np_binarize(x_host_np.reshape(-1))
    flag = buf.flag.item()
    assert flag == flag_ref, (what, "flag", flag, "numpy", flag_ref)
    occ = buf.occ.cpu().numpy()
    bad = np.nonzero(occ != occ_ref)[0]
    assert bad.size == 0, (what, "occ differs at", bad[:8].tolist(), occ[bad[:8]].tolist(), occ_ref[bad[:8]].tolist())
    assert buf.guard_intact(), (what, "bytes behind occ_ws were written")
    return flag_ref


def _unit_bank(dev):
    return torch.full((1, 1, 1, 1), 0.75, device=dev), torch.ones(1, device=dev)


# ------------------------------------------------------------------------------------------------------------------ 0.
def test_out_dtype_is_refused_before_anything_is_launched(hip_device):
    """SN_BF16 used to reach conv_bank_group's refusal with binarize_kernel and the linear kernel already enqueued"""
    r = fc.ROUTES["lin24-G16"]
    bank, lam = (t.to(hip_device) for t in fc.bank_of("lin24-G16", fc.SPANS[0]))
    x = fc.grid_of(r.shape, "binary").to(hip_device)
    buf = Buffers(r.shape, torch.float32, hip_device)        # (bf16 needs half of it)
    for code in (_hip.SN_BF16, _hip.SN_U8, _hip.SN_I32):
        rc = _raw(x, bank, lam, buf, out_code=code)
        assert rc == -1 and b"out_dtype" in _hip.load().sn_last_error(), (code, rc, _hip.load().sn_last_error())
    torch.cuda.synchronize()
    assert buf.flag.item() == fc.FLAG_POISON and bool((buf.occ_all == fc.OCC_POISON).all()) and bool(buf.out.isnan().all())
    with pytest.raises(_hip.HipLibraryError, match="out_dtype"):
        _hip.forward_auto(x, bank, lam, out_dtype=torch.bfloat16)
    assert _hip.device_status()[0] == 0


# ------------------------------------------------------------------------------------------------------------------ B.
@pytest.mark.parametrize("dt", fc.DTYPES, ids=["f32", "f64"])
def test_binarize_base_grid_and_poisoned_buffers(hip_device, dt):
    """zeros and ones at density 0.2: flag 0, every byte of occ rewritten, nothing behind it"""
    bank, lam = _unit_bank(hip_device)
    for shape in ((1, 1, 1, 1, 1399), (3, 1, 5, 3, 7), (1, 1, 1, 1, 1), (1, 1, 1, 1, 2), (1, 1, 1, 1, 3), (2, 1, 9, 17, 68)):
        xh = fc.binary_grid(shape, 0.2, 7).astype(fc.NP_OF[dt])
        buf = _auto(torch.from_numpy(xh).to(hip_device), bank, lam, dt)
        assert _check_classification(buf, xh, shape) == 0
        occ = buf.occ.cpu().numpy()
        assert set(np.unique(occ).tolist()) <= {0, 1}
        # the 1 x 1 x 1 forward: relu(tanh(0.75 x)) -- the int8 form ran (flag 0) and wrote every voxel
        want = np.tanh(0.75) * xh.astype(np.float64)
        assert np.abs(buf.out.cpu().double().numpy() - want).max() < TOL, shape


@pytest.mark.parametrize("dt", fc.DTYPES, ids=["f32", "f64"])
def test_binarize_one_odd_value_at_every_position_class(hip_device, dt):
    """an otherwise binary grid with one table value at one position: flag and every byte of occ are numpy's"""
    bank, lam = _unit_bank(hip_device)
    npdt = fc.NP_OF[dt]
    table = fc.odd_values(npdt)
    for pos in fc.positions():
        base = fc.binary_grid(pos.shape, 0.2, 11).astype(npdt)
        buf = Buffers(pos.shape, dt, hip_device)
        for name, v in table:
            xh = base.copy()
            xh.reshape(-1)[pos.index] = v
            x = torch.from_numpy(xh).to(hip_device)
            assert _same_bits(x.cpu(), torch.from_numpy(xh)), "the value did not survive the copy"
            buf.poison()
            _auto(x, bank, lam, dt, buf)
            flag = _check_classification(buf, xh, (pos.name, name, dt))
            assert flag == (0 if name in ("+0", "-0", "1") else 1), (pos.name, name)
            assert buf.occ[pos.index].item() == (0 if name in ("+0", "-0") else 1), (pos.name, name)
    assert _hip.device_status()[0] == 0


@pytest.mark.parametrize("dt", fc.DTYPES, ids=["f32", "f64"])
def test_binarize_second_trip_of_the_grid_stride_loop(hip_device, dt):
    """2 108 160 elements under a 1 x 1 x 1 bank: indices from 2048 * 256 * 4 on are reached by the loop's second trip only"""
    bank, lam = _unit_bank(hip_device)
    npdt = fc.NP_OF[dt]
    assert _hip.conv_fused_supported(torch.zeros(fc.BIG, dtype=torch.bool), (1, 1, 1))
    base = fc.binary_grid(fc.BIG, 0.2, 13).astype(npdt)
    occ_base, flag_base = fc.np_binarize(base.reshape(-1))
    assert flag_base == 0
    x = torch.from_numpy(base).to(hip_device)
    occ_ref = torch.from_numpy(occ_base).to(hip_device)
    buf = _auto(x, bank, lam, dt)
    assert buf.flag.item() == 0 and torch.equal(buf.occ, occ_ref) and buf.guard_intact()
    assert not buf.out.isnan().any().item()
    assert torch.equal(buf.out.view(-1) != 0, occ_ref != 0)
    for pos in fc.big_positions():
        for name, v in fc.odd_values(npdt):
            one = np.array([v], dtype=npdt)
            o1, f1 = fc.np_binarize(one)
            x.view(-1)[pos.index:pos.index + 1] = torch.from_numpy(one).to(hip_device)
            occ_ref[pos.index] = int(o1[0])
            buf.poison()
            _auto(x, bank, lam, dt, buf)
            assert buf.flag.item() == f1, (pos.name, name, buf.flag.item(), f1)
            assert torch.equal(buf.occ, occ_ref), (pos.name, name, _first_difference(buf.occ, occ_ref))
            assert buf.guard_intact()
        x.view(-1)[pos.index] = float(base.reshape(-1)[pos.index])
        occ_ref[pos.index] = int(occ_base[pos.index])
    assert _hip.device_status()[0] == 0


# ------------------------------------------------------------------------------------------------------------------ C.
def _int8_form(xb, bank, lam, out_dtype, route):
    """the byte form by its own entries: the linear kernel where it serves the shape, else sn_conv_bank on the bool grid"""
    if route.fused:
        assert _hip.conv_fused_supported(xb, route.ks)
        return _hip.conv_fused(xb, bank, lam, out_dtype=out_dtype)
    assert not _hip.conv_fused_supported(xb, route.ks)
    return _hip.conv_bank(xb, bank, lam, want_act=False, out_dtype=out_dtype)[1]


def _verdict(xb, bank, lam):
    v = torch.full((1,), -1, dtype=torch.int32, device=xb.device)
    _hip.conv_fused(xb, bank, lam, verdict=v)
    return v.item()


def _route_case(name, kind, declined, dev, variant=0):
    """One row of the table for x in f32 and f64 and out in f32 and f64.  kind: 'binary' | 'half' | 'uniform' | 'nan'."""
    route = fc.ROUTES[name]
    assert fc.route_plan(name) == (route.fused, route.bool_kernel, route.w24), (name, fc.route_plan(name))
    xh = fc.grid_of(route.shape, kind, variant)
    flag_ref = fc.np_binarize(xh.numpy())[1]
    assert flag_ref == (0 if kind == "binary" else 1)
    forms_differ = not (kind == "binary" and not declined and route.bool_kernel == "fp32")
    span_used = None
    for span in fc.SPANS:
        bank, lam = (t.to(dev) for t in fc.bank_of(name, span))
        x32 = xh.to(dev)
        xb = x32 != 0
        if kind == "binary":
            if declined:   # the fp32 kernel on the bytes must win over the int8 kernels (default tolerance: they serve)
                winner = _hip.conv_bank(x32.to(torch.uint8), bank, lam, want_act=False, out_dtype=torch.float32)[1]
                other = _int8_form(xb, bank, lam, torch.float32, route)
            else:          # the int8 form must win over the fp32 contraction of the floats
                winner = _int8_form(xb, bank, lam, torch.float32, route)
                other = _hip.conv_bank(x32, bank, lam, want_act=False, out_dtype=torch.float32)[1]
        else:              # the fp32 contraction of x itself must win over the int8 form of (x != 0)
            winner = _hip.conv_bank(x32, bank, lam, want_act=False, out_dtype=torch.float32)[1]
            other = _int8_form(xb, bank, lam, torch.float32, route)
        if not forms_differ or not _same_bits(winner, other):
            span_used = span
            break
    assert span_used is not None, (name, kind, "the two forms agree in every bit at every span: nothing tells them apart")
    if route.fused and kind == "binary":   # the guard's verdict, read where the linear kernel serves the shape
        assert _verdict(xb, bank, lam) == 0, (name, "the guard declines at the default tolerance")
        if declined:
            with _hip.options(**fc.DECLINE):
                assert _verdict(xb, bank, lam) == 1, (name, "the guard serves at 1 ppb")
    ref = fc.oracle_out(name, span_used, kind, variant) if kind != "nan" else None
    for xdt in fc.DTYPES:
        x = xh.to(xdt).to(dev)
        for odt in fc.DTYPES:
            what = (name, kind, "declined" if declined else "served", xdt, odt, span_used)
            if kind == "binary" and declined:
                want = _hip.conv_bank(x.to(torch.uint8), bank, lam, want_act=False, out_dtype=odt)[1]
            elif kind == "binary":
                want = _int8_form(x.bool(), bank, lam, odt, route)
            else:
                want = _hip.conv_bank(x, bank, lam, want_act=False, out_dtype=odt)[1]
            with _hip.options(**(fc.DECLINE if declined else {})):
                buf = _auto(x, bank, lam, odt)
            assert buf.flag.item() == flag_ref, what
            assert buf.guard_intact() and torch.equal(buf.occ, (x != 0).view(-1).to(torch.uint8)), what
            if kind == "nan":
                assert torch.equal(buf.out.isnan(), want.isnan()) and buf.out.isnan().any().item(), what
                assert buf.out.isnan().sum().item() <= int(np.prod(route.ks)), what
                assert _same_bits(buf.out, want), (what, "bits outside the NaN pattern")
                continue
            assert not buf.out.isnan().any().item(), (what, "NaN left in out", int(buf.out.isnan().sum()))
            assert torch.equal(buf.out, want), (what, _first_difference(buf.out, want))
            err = (buf.out.cpu().double() - ref).abs().max().item()
            assert err < TOL, (what, err)
    assert _hip.device_status()[0] == 0


@pytest.mark.parametrize("name", fc.BINARY_ROUTES)
def test_binary_grids_take_the_byte_form(hip_device, name):
    _route_case(name, "binary", False, hip_device)


@pytest.mark.parametrize("name", fc.DECLINED_ROUTES)
def test_declined_guard_sends_binary_grids_to_the_fp32_kernel_on_the_bytes(hip_device, name):
    """conv_i8_tolerance_ppb = 1: the nested gate, "binary AND verdict == 1\""""
    _route_case(name, "binary", True, hip_device)


@pytest.mark.parametrize("kind", ["half", "uniform"])
@pytest.mark.parametrize("name", fc.NONBINARY_ROUTES)
def test_other_grids_take_the_fp32_contraction(hip_device, name, kind):
    _route_case(name, kind, False, hip_device)


@pytest.mark.parametrize("name", ["lin24-G4", "four-copy-G20", "ragged-5x7x9-G4"])
def test_a_nan_in_x_comes_back_as_conv_banks_nan_pattern(hip_device, name):
    _route_case(name, "nan", False, hip_device)


# ------------------------------------------------------------------------------------------------------------------ D.
def _alone(x, bank, lam, odt, declined):
    with _hip.options(**(fc.DECLINE if declined else {})):
        buf = _auto(x, bank, lam, odt)
    torch.cuda.synchronize()
    return buf


@pytest.mark.parametrize("name", ["lin24-G16", "four-copy-G20"])
def test_eight_calls_back_to_back_equal_the_calls_alone(hip_device, name):
    """binary and non-binary in turn, a guard-declined bank in the middle, one synchronisation at the end: a verdict word
    from the recycled ring that one call left behind must not decide another's"""
    route = fc.ROUTES[name]
    bank, lam = (t.to(hip_device) for t in fc.bank_of(name, fc.SPANS[0]))
    kinds = [("binary", 0, False), ("half", 1, False), ("binary", 2, False), ("uniform", 3, False), ("binary", 4, True),
             ("half", 5, True), ("binary", 6, False), ("nan", 7, False)]
    calls = []
    for i, (kind, variant, declined) in enumerate(kinds):
        dt = fc.DTYPES[i % 2]
        odt = fc.DTYPES[(i // 2) % 2]
        calls.append((fc.grid_of(route.shape, kind, variant).to(dt).to(hip_device), odt, declined))
    alone = [_alone(x, bank, lam, odt, declined) for x, odt, declined in calls]
    assert [b.flag.item() for b in alone] == [0, 1, 0, 1, 0, 1, 0, 1]
    bufs = [Buffers(route.shape, odt, hip_device) for _, odt, _ in calls]
    torch.cuda.synchronize()
    for (x, _, declined), buf in zip(calls, bufs):
        with _hip.options(**(fc.DECLINE if declined else {})):
            rc = _raw(x, bank, lam, buf)
        assert rc == 0, _hip.load().sn_last_error()
    torch.cuda.synchronize()
    for i, (buf, ref) in enumerate(zip(bufs, alone)):
        assert buf.flag.item() == ref.flag.item(), (name, i)
        assert torch.equal(buf.occ_all, ref.occ_all), (name, i)
        assert _same_bits(buf.out, ref.out), (name, i, kinds[i])
    assert _hip.device_status()[0] == 0


# ------------------------------------------------------------------------------------------------------------------ E.
@pytest.mark.parametrize("name", ["lin24-G16", "four-copy-G4"])
@pytest.mark.parametrize("dt", fc.DTYPES, ids=["f32", "f64"])
def test_a_captured_call_replays_while_the_content_changes_class(hip_device, name, dt):
    """x, occ_ws, the flag and out are static; before each replay out is refilled with NaN and the flag set to -7: the
    memset node resets it on every replay, and neither form's launches leak into the other's turn"""
    route = fc.ROUTES[name]
    bank, lam = (t.to(hip_device) for t in fc.bank_of(name, fc.SPANS[0]))
    turns = [("binary", 0), ("half", 1), ("binary", 0), ("binary", 2), ("nan", 3)]
    grids = [fc.grid_of(route.shape, k, v).to(dt).to(hip_device) for k, v in turns]
    eager = [_alone(x, bank, lam, dt, False) for x in grids]
    assert [b.flag.item() for b in eager] == [0, 1, 0, 0, 1]
    assert not _same_bits(eager[0].out, eager[3].out) and not _same_bits(eager[0].out, eager[1].out)
    x = grids[0].clone()
    buf = Buffers(route.shape, dt, hip_device)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        assert _raw(x, bank, lam, buf) == 0      # warm-up on the capturing stream: attributes, pools
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        rc = _raw(x, bank, lam, buf)
    assert rc == 0, _hip.load().sn_last_error()
    for i, (g, ref) in enumerate(zip(grids, eager)):
        x.copy_(g)
        buf.poison()
        graph.replay()
        torch.cuda.synchronize()
        assert buf.flag.item() == ref.flag.item(), (name, "replay", i, buf.flag.item())
        assert torch.equal(buf.occ_all, ref.occ_all), (name, "replay", i)
        assert _same_bits(buf.out, ref.out), (name, "replay", i, turns[i])
    assert _hip.device_status()[0] == 0


# ------------------------------------------------------------------------------------------------------------------ F.
def test_wrapper_on_a_view_that_is_not_16_byte_aligned(hip_device):
    bank, lam = (t.to(hip_device) for t in fc.bank_of("ragged-5x7x9-G4", fc.SPANS[0]))
    for kind in ("binary", "half"):
        full = fc.grid_of((3, 1, 5, 7, 9), kind, 5).to(hip_device)       # 315 floats per element
        view = full[1:]
        assert view.data_ptr() % 16 != 0 and view.is_contiguous()
        out_v, flag_v = _hip.forward_auto(view, bank, lam)
        out_c, flag_c = _hip.forward_auto(view.clone(), bank, lam)
        assert flag_v.item() == flag_c.item() == fc.np_binarize(view.cpu().numpy())[1]
        assert torch.equal(out_v, out_c) and not out_v.isnan().any().item()
        assert torch.equal(out_c, _auto(view.clone(), bank, lam, torch.float32).out)


@functools.lru_cache(maxsize=None)
def _model(dev):
    torch.manual_seed(21)
    return sna.SceneNet({"cy": 2, "cone": 1, "neg": 1}, (9, 9, 9)).to(dev)


def _oracle_forward(model, x64):
    from oracle import geneo_oracle as go
    names = list(model.geneos.keys())
    specs = [(n.split("_")[0], {k: float(v) for k, v in model.geneos[n].geneo_params.items()}) for n in names]
    lam = [float(model.lambdas_dict[f"lambda_{n}"]) for n in names]
    last = names.index(model.last_lambda.replace("lambda_", ""))
    return go.scenenet_forward(x64, specs, model.kernel_size_of_bank(), lam, last, names=names)


def test_module_in_eval_routes_f64_occupancy_through_the_byte_form(hip_device):
    model = _model(str(hip_device)).eval()
    x = fc.grid_of(fc.ROW1, "binary", 9).double().to(hip_device)
    assert _hip.conv_fused_supported(x.bool(), (9, 9, 9))
    with torch.no_grad():
        out = model(x)
        assert out.dtype == torch.float64 and torch.equal(out, model(x.bool()).to(torch.float64))
        xr = fc.grid_of(fc.ROW5A, "binary", 9).double()
        outr = model(xr.to(hip_device))
        assert (outr.cpu() - _oracle_forward(model, xr)).abs().max().item() < TOL
        assert (out.cpu() - _oracle_forward(model, x.cpu())).abs().max().item() < TOL


@pytest.mark.parametrize("kind", ["binary", "half"])
def test_module_under_autograd_routes_float_grids_through_it(hip_device, kind):
    """out is forward_auto's; every trainable scalar gets a finite gradient (their values: test_gpu_backward.py)"""
    model = _model(str(hip_device)).train()
    x = fc.grid_of(fc.ROW1, kind, 9).double().to(hip_device)
    params = [p for p in model.parameters() if p.requires_grad]
    assert params
    for p in params:
        p.grad = None
    out = model(x)
    assert out.requires_grad and out.dtype == torch.float64
    saved = out.grad_fn.saved_tensors       # (x, out, bank, P, lam, kinds): the bank and coefficients this forward built
    bank, lam = saved[2], saved[4]
    assert tuple(bank.shape) == (4, 9, 9, 9) and tuple(lam.shape) == (4,)
    with torch.no_grad():
        want, flag = _hip.forward_auto(x, bank, lam)
    assert flag.item() == (0 if kind == "binary" else 1)
    assert torch.equal(out.detach(), want)
    out.sum().backward()
    for p in params:
        assert p.grad is not None and torch.isfinite(p.grad).all().item()
    assert any(p.grad.abs().max().item() > 0 for p in params)
    assert _hip.device_status()[0] == 0
