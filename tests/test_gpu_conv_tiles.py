"""sn_conv_bank at every workgroup tile its four kernels can pick, on the MI355X.

The fp32 MFMA kernel (csrc/conv_fp32.inc), the four-copy int8 kernel (conv_i8.hip, staged and unstaged templates), the
stride-4 int8 kernel and its folded form (conv_i8s.hip) choose their tile from one ladder, {8,8} {4,8} {4,4} {2,4} {1,4}
{1,2} (TZ, TX; TY = 64): the first rung that fits LDS and yields 4 tiles per compute unit.  Small grids only ever reach the
bottom of it.  Here the batch size is SEARCHED with the library's own plan query (sn_conv_bank_plan) until a grid whose
extents are multiples of no tile (61 x 59 x 132, 30 x 59 x 132, 7 x 5 x 68, 5 x 13 x 68 -- and x 144 / x 80 where the
stride-4 kernel wants Y % 16 == 0) lands on the wanted rung of the device at hand; every case then asserts, sharpest first:

a. batch independence, bit for bit: each element (eight of them where B > 8) run alone -- a small rung -- equals its slice
   of the big-tile run.  The accumulation order of a voxel is the tap table's (conv_fp32.inc: tap steps t = 0 .. T4 - 1 of
   one accumulator, four taps per MFMA; int8: exact integers), never the tile's, so equality is required for fp32 too;
b. variant equality at the same shape: staged == unstaged, four-copy == stride-4 == folded, double-buffered ==
   single-buffered, conv_no_i8 == the fp32 kernel on the bytes, the guard's fp32 route == the fp32 kernel called directly;
c. the fp64 oracle on whole batch elements (first, last, the completely full one; three of the 5 x 13 x 68 batch):
   int8 with the project's bars as they stand (conftest.act_err_ok, the analytic quantisation bound of
   test_gpu_conv_i8_envelope.py -- with max|ref| taken over the element compared, never more than that test's --, 1e-4 on
   the output); fp32 with the former whole-tensor bar 1e-4 * max(1, max|ref|) as an outer bar and, elementwise,

       |act - ref|[v] <= C * sqrt(T) * 2^-24 * (|x| * |w|)[v] + 1e-30,     T = kz kx ky,  (|x| * |w|) in fp64 by the oracle.

C was measured on a CPU, not on the kernel: an fp32 emulation of the reference operation (one fp32 accumulator, the
product rounded, taps in table order; randn input given as f32 and as f64 rounded on load, weights uniform in +-0.5, a
10^3 grid, 8 seeds) against fp64 gave as largest ratio |emu - ref| / (sqrt(T) 2^-24 (|x| * |w|)):
    (9,9,9) 0.131   (9,5,5) 0.198   (9,7,7) 0.161   (6,5,6) 0.278   (3,3,17) 0.332   [(3,3,25) 0.201]
The largest over the sizes used here, 0.332, times 4 (the MFMA adds the four products of a step in an order of its own,
and the maximum here runs over 10^6 voxels, not 10^3):  C = 1.328.  The worst-case bound (T + 2) 2^-24 (|x| * |w|) is 20
to 200 times looser and pins nothing.

The last test of the module checks coverage: for each kernel form, every rung the plan query can reach with one of the
tested kernel sizes was run; the rungs a form cannot reach are named there."""
import zlib

import numpy as np
import pytest
import torch

from scene_net_amd import _hip
from oracle import geneo_oracle as go

from conftest import act_err_ok
from test_gpu_conv_i8_envelope import quant_bound

pytestmark = pytest.mark.gpu
TOL = 1e-4
C_FP32 = 4 * 0.332
RUNGS = [(8, 8), (4, 8), (4, 4), (2, 4), (1, 4), (1, 2)]
SIZES = [((9, 9, 9), 16), ((9, 5, 5), 3), ((9, 7, 7), 5), ((6, 5, 6), 5), ((3, 3, 17), 2), ((9, 9, 9), 20)]
# extents that are multiples of no tile; the second family has the y tiles of the first and Y % 16 == 0
RAGGED = {4: [(61, 59, 132), (30, 59, 132), (7, 5, 68)], 16: [(61, 59, 144), (30, 59, 144), (7, 5, 80)]}
THIN = {4: (5, 13, 68), 16: (5, 13, 80)}      # smaller than the big tile in z, Y = 64 + 4 (+ 16)
MAX_BYTES = 1e9                                # of one tensor (the f64 activations)

F32_SINGLE, F32_DOUBLE = "fp32 single-buffered", "fp32 double-buffered"
I8_STAGED, I8_UNSTAGED = "four-copy staged", "four-copy unstaged"
I8_STRIDE4, I8_FOLDED = "stride-4", "folded"
FORMS = [F32_SINGLE, F32_DOUBLE, I8_STAGED, I8_UNSTAGED, I8_STRIDE4, I8_FOLDED]
# how a form is asked for: (x dtype, options)
FORM_OPTS = {
    F32_SINGLE: (torch.float32, dict(conv_double_buffer=0)),
    F32_DOUBLE: (torch.float32, dict(conv_double_buffer=1)),
    I8_STAGED: (torch.bool, dict(conv_i8_legacy=1, conv_i8_no_stage=0)),
    I8_UNSTAGED: (torch.bool, dict(conv_i8_legacy=1, conv_i8_no_stage=1)),
    I8_STRIDE4: (torch.bool, dict(conv_i8_legacy=0, conv_i8_fold=0)),
    I8_FOLDED: (torch.bool, dict(conv_i8_legacy=0, conv_i8_fold=1)),
}
RAN = {}        # (form, rung) -> cases that launched it
CASES_RUN = set()


def _form_of(plan):
    if plan.kernel == "fp32":
        return F32_DOUBLE if plan.double_buffered else F32_SINGLE
    if plan.kernel == "four_copy":
        return I8_STAGED if plan.staged else I8_UNSTAGED
    return I8_STRIDE4 if plan.kernel == "stride4" else I8_FOLDED


def _plan(dtype, B, grid, bank_shape, opts):
    with _hip.options(**opts):
        return _hip.conv_bank_plan((dtype, (B, 1) + tuple(grid)), bank_shape)


def _find(form, ks, G, rung, grids):
    """(B, grid): the smallest batch of the first grid for which `form` plans `rung` on this device; None if there is none"""
    dtype, opts = FORM_OPTS[form]
    want = RUNGS.index(rung)
    for grid in grids:
        for B in range(1, 2049):
            if B * G * grid[0] * grid[1] * grid[2] * 8 > MAX_BYTES:
                break
            p = _plan(dtype, B, grid, (G,) + ks, opts)
            if _form_of(p) != form:
                continue       # not this form at this batch size (the staged template: at the big tile only)
            at = RUNGS.index(p.rung)
            if at == want:
                return B, grid
            if at < want:
                break          # more tiles only climb the ladder
    return None


def _run(x, bank, lam, what, opts, note=True, **kw):
    """conv_bank under `opts`; what the plan query says was launched goes into the coverage table"""
    with _hip.options(**opts):
        p = _hip.conv_bank_plan(x, tuple(bank.shape))
        act, out = _hip.conv_bank(x, bank, lam, want_act=kw.pop("want_act", True), want_out=True, **kw)
    if note:
        RAN.setdefault((_form_of(p), p.rung), []).append(what)
    return act, out, p


def _same(a, b, what):
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), what


def _alone(x, B):
    return sorted(set(range(B)) if B <= 8 else set(np.linspace(0, B - 1, 8).round().astype(int).tolist()))


def _check_batch_independence(x, bank, lam, got, opts, what, **kw):
    """each element alone (B = 1: a small rung) == its slice of the big run, bit for bit"""
    B = x.shape[0]
    if B == 1:
        return
    for b in _alone(x, B):
        a1, o1, p1 = _run(x[b:b + 1].clone(), bank, lam, what, opts, note=False, **kw)
        assert torch.equal(a1[0], got[0][b]) and torch.equal(o1[0], got[1][b]), (what, "element", b, p1)


def _oracle_elements(B, thin, extra=()):
    els = {0, B - 1} | set(extra)
    if thin:
        els.add((B - 1) // 2)
    return sorted(els)


def _ref(xb, bank, lam):
    G = bank.shape[0]
    ref_act = go.conv_bank(xb.double(), bank.double().unsqueeze(1))
    ref_out = torch.relu(torch.tanh((lam.double().view(1, G, 1, 1, 1) * ref_act).sum(1, keepdim=True)))
    return ref_act, ref_out


def _symmetric(bank):
    """bit-for-bit symmetric in x and y (what the folded kernel asks for): mirror copies, no arithmetic"""
    b = bank.clone()
    kx, ky = b.shape[2], b.shape[3]
    b[:, :, kx - kx // 2:, :] = b[:, :, :kx // 2, :].flip(2)
    b[:, :, :, ky - ky // 2:] = b[:, :, :, :ky // 2].flip(3)
    return b


def _cases(sizes, fams):
    out = []
    for ks, G in sizes:
        rungs = RUNGS[:3] if G > 16 else RUNGS      # two kernel groups: the big tiles (partial sums carried in `out`)
        for fam in fams(ks):
            out += [(ks, G, fam, r, False) for r in rungs] + [(ks, G, fam, RUNGS[0], True)]
    return out


def _id(c):
    ks, G, fam, rung, thin = c
    return f"{ks[0]}x{ks[1]}x{ks[2]}-G{G}-Y%{fam}-{'thin-' if thin else ''}{rung[0]}x{rung[1]}"


# --------------------------------------------------------------------------------------------------------------- fp32
FP32_CASES = [c + (d,) for c in _cases(SIZES, lambda ks: [4]) for d in (False, True)]


@pytest.mark.parametrize("case", FP32_CASES, ids=lambda c: _id(c[:5]) + ("-double" if c[5] else "-single"))
def test_fp32_kernel_at_every_rung(hip_device, case):
    ks, G, fam, rung, thin, dbl = case
    form = F32_DOUBLE if dbl else F32_SINGLE
    what = _id(case[:5]) + ("-double" if dbl else "-single")
    CASES_RUN.add(("fp32", case))
    found = _find(form, ks, G, rung, [THIN[fam]] if thin else RAGGED[fam])
    if found is None:       # not a rung of this form at this kernel size (LDS, staging registers): see the coverage test
        return
    B, grid = found
    g = torch.Generator().manual_seed(zlib.crc32(what.encode()) % 2**31)
    x64 = torch.randn((B, 1) + grid, generator=g, dtype=torch.float64)
    bank = torch.rand((G,) + ks, generator=g) - 0.5
    lam = (torch.rand(G, generator=g) - 0.3) / G
    bd, ld = bank.to(hip_device).contiguous(), lam.to(hip_device)
    x = x64.float().to(hip_device)
    single, double = FORM_OPTS[F32_SINGLE][1], FORM_OPTS[F32_DOUBLE][1]

    got = _run(x, bd, ld, what, FORM_OPTS[form][1])
    assert _form_of(got[2]) == form and got[2].rung == rung, got[2]
    # b. the other buffering at the same shape (whatever rung it takes there), and f64 storage of the same fp32 numbers
    other = _run(x, bd, ld, what, single if dbl else double)
    _same(got, other, (what, "double- vs single-buffered", got[2], other[2]))
    del other
    o64 = _run(x, bd, ld, what, FORM_OPTS[form][1], out_dtype=torch.float64)
    assert torch.equal(o64[0], got[0].double()) and torch.equal(o64[1], got[1].double()), (what, "f64 output")
    del o64
    # a.
    _check_batch_independence(x, bd, ld, got, single, what)
    # c.
    T = ks[0] * ks[1] * ks[2]
    runs = [("f32 in", x64.float(), got)]
    if not dbl:     # genuine f64 input (rounded to fp32 on load), both output types
        xd = x64.to(hip_device)
        g64 = _run(xd, bd, ld, what, single, out_dtype=torch.float64)
        g6432 = _run(xd, bd, ld, what, single, out_dtype=torch.float32)
        assert torch.equal(g64[0], g6432[0].double()) and torch.equal(g64[1], g6432[1].double()), (what, "f64 in")
        _same(g6432, got, (what, "f64 input rounds to the f32 input's bits"))     # x64.float() is that rounding
        del g6432
        runs.append(("f64 in", x64, g64))
    for tag, xin, res in runs:
        for b in _oracle_elements(B, thin):
            ref_act, ref_out = _ref(xin[b:b + 1], bank, lam)
            mag = go.conv_bank(xin[b:b + 1].double().abs(), bank.double().abs().unsqueeze(1))
            err = (res[0][b:b + 1].cpu().double() - ref_act).abs()
            ratio = (err / (np.sqrt(T) * 2.0 ** -24 * mag + 1e-30)).max().item()
            e_out = (res[1][b:b + 1].cpu().double() - ref_out).abs().max().item()
            print(f"{what} B={B} {grid} {tag} element {b}: max err {err.max().item():.2e}, elementwise ratio "
                  f"{ratio:.3f} (bar {C_FP32}), out err {e_out:.2e}")
            assert err.max().item() < TOL * max(1.0, ref_act.abs().max().item()), (what, tag, b)
            assert ratio <= C_FP32, (what, tag, b, ratio)
            assert e_out < TOL, (what, tag, b, e_out)


# --------------------------------------------------------------------------------------------------------------- int8
def _nine(ks):
    return ks[2] == 9 and ks[0] * ks[1] == 81


I8_CASES = _cases(SIZES, lambda ks: [4, 16] if _nine(ks) else [4])


def _occupancy(B, grid, g):
    x = torch.rand((B, 1) + grid, generator=g) < 0.3
    full = None
    if B >= 3:
        full = 1
        x[full] = True
        x[B - 2 if B > 3 else 2] = False
    return x, full


def _int8_oracle(res, x, bank, lam, els, what):
    bounds = [quant_bound(bank[g].numpy()) for g in range(bank.shape[0])]
    for b in els:
        ref_act, ref_out = _ref(x[b:b + 1], bank, lam)
        act = res[0][b:b + 1].cpu().double()
        assert act_err_ok(act, ref_act, TOL), (what, b)
        worst = 0.0
        for g in range(bank.shape[0]):
            amax = ref_act[:, g].abs().max().item()
            err = (act[:, g] - ref_act[:, g]).abs().max().item()
            worst = max(worst, err)
            assert err < TOL * max(1.0, amax), (what, b, g, err, amax)
            assert err <= bounds[g] + 4e-7 * max(1.0, amax), (what, b, g, err, bounds[g])
        e_out = (res[1][b:b + 1].cpu().double() - ref_out).abs().max().item()
        print(f"{what} element {b}: max act err {worst:.2e} (largest bound {max(bounds):.2e}), out err {e_out:.2e}")
        assert e_out < TOL, (what, b, e_out)


@pytest.mark.parametrize("case", I8_CASES, ids=_id)
def test_int8_kernels_at_every_rung(hip_device, case):
    ks, G, fam, rung, thin = case
    what = _id(case)
    CASES_RUN.add(("int8", case))
    lead = I8_STRIDE4 if fam == 16 else I8_UNSTAGED        # the form whose ladder the batch size is searched on
    found = _find(lead, ks, G, rung, [THIN[fam]] if thin else RAGGED[fam])
    if found is None:
        return
    B, grid = found
    g = torch.Generator().manual_seed(zlib.crc32(what.encode()) % 2**31)
    occ, full = _occupancy(B, grid, g)
    bank = (torch.rand((G,) + ks, generator=g) - 0.5) * torch.logspace(-2, 0.3, G).view(G, 1, 1, 1)
    lam = (torch.rand(G, generator=g) - 0.3) / G
    # this test's own precondition: the guard keeps these banks on the int8 kernels (it would route them to fp32 silently)
    tol_dev = 1e-9 * _hip.get_option("conv_i8_tolerance_ppb")
    for bk in (bank, _symmetric(bank)):
        bounds = np.array([quant_bound(bk[i].numpy()) for i in range(G)])
        assert bounds.max() < 0.5 * tol_dev and float((lam.abs().double().numpy() * bounds).sum()) < 0.5 * tol_dev
    x, bd, ld = occ.to(hip_device), bank.to(hip_device).contiguous(), lam.to(hip_device)
    spins0 = _hip.conv_i8_spin_timeouts()
    ngroups = (G + 15) // 16
    els = _oracle_elements(B, thin, [] if full is None else [full])

    # b. the four-copy kernel, unstaged and (at the big tile, rows of <= 80 bytes) staged
    uns = _run(x, bd, ld, what, FORM_OPTS[I8_UNSTAGED][1])
    assert _form_of(uns[2]) == I8_UNSTAGED, uns[2]
    stg = _run(x, bd, ld, what, FORM_OPTS[I8_STAGED][1])
    # rows of (3,3,17) need 86 bytes (> 80): unstaged at every tile; every other size here is staged at the big tile
    assert stg[2].kernel == "four_copy" and stg[2].staged == (stg[2].rung == (8, 8) and ks != (3, 3, 17)), stg[2]
    _same(uns, stg, (what, "staged vs unstaged", stg[2], uns[2]))
    out_only = _run(x, bd, ld, what, FORM_OPTS[I8_STAGED][1], want_act=False)
    assert out_only[0] is None and torch.equal(out_only[1], uns[1]), (what, "out only")
    del stg, out_only
    if lead == I8_UNSTAGED:
        assert uns[2].rung == rung, uns[2]
    for form in (I8_STAGED, I8_UNSTAGED):       # f64 storage: the double templates
        r64 = _run(x, bd, ld, what, FORM_OPTS[form][1], out_dtype=torch.float64)
        assert torch.equal(r64[0], uns[0].double()) and torch.equal(r64[1], uns[1].double()), (what, form, "f64 output")
        del r64
    # the stride-4 kernel on its own, and as the body the folded launch runs for a bank that is not symmetric
    if fam == 16:
        s4 = _run(x, bd, ld, what, FORM_OPTS[I8_STRIDE4][1])
        assert _form_of(s4[2]) == I8_STRIDE4 and s4[2].rung == rung, s4[2]
        _same(uns, s4, (what, "four-copy vs stride-4", s4[2]))
        c0 = _hip.conv_i8_path_counts()
        dec = _run(x, bd, ld, what, FORM_OPTS[I8_FOLDED][1], note=False)     # declined on the device: the stride-4 body
        c1 = _hip.conv_i8_path_counts()
        if dec[2].kernel == "folded":
            assert (c1[0] - c0[0], c1[1] - c0[1], c1[2] - c0[2]) == (0, ngroups, 0), (what, c0, c1)
            RAN.setdefault((I8_STRIDE4, dec[2].rung), []).append(what + " (body of the folded launch)")
        _same(uns, dec, (what, "four-copy vs the folded launch's stride-4 body", dec[2]))
        s464 = _run(x, bd, ld, what, FORM_OPTS[I8_STRIDE4][1], out_dtype=torch.float64)
        assert torch.equal(s464[0], uns[0].double()) and torch.equal(s464[1], uns[1].double()), (what, "stride-4 f64")
        del s4, dec, s464
    # conv_no_i8 and the guard's route: the fp32 kernel's bits
    f32 = _run(x.view(torch.uint8), bd, ld, what + " (u8)", FORM_OPTS[F32_SINGLE][1])
    no_i8 = _run(x, bd, ld, what + " (conv_no_i8)", dict(conv_no_i8=1, conv_double_buffer=0))
    assert no_i8[2].kernel == "fp32", no_i8[2]
    _same(f32, no_i8, (what, "conv_no_i8"))
    del no_i8
    for legacy in ([0, 1] if fam == 16 else [1]):
        routed = _run(x, bd, ld, what, dict(conv_i8_tolerance_ppb=1, conv_i8_legacy=legacy, conv_double_buffer=0),
                      note=False)
        _same(f32, routed, (what, "guard route, legacy =", legacy))
        del routed
    RAN.setdefault((F32_SINGLE, f32[2].rung), []).append(what + " (the guard's fp32 route)")
    del f32
    # a. (under the defaults: the folded launch where it serves the shape, else the four-copy kernel)
    _check_batch_independence(x, bd, ld, uns, {}, what)
    # c.
    _int8_oracle(uns, occ, bank, lam, els, what)
    del uns

    # the folded kernel proper: a symmetric bank, served on the device
    if fam == 16:
        sym = _symmetric(bank)
        sd = sym.to(hip_device).contiguous()
        ref4 = _run(x, sd, ld, what + " (symmetric bank)", FORM_OPTS[I8_UNSTAGED][1])
        c0 = _hip.conv_i8_path_counts()
        fol = _run(x, sd, ld, what, FORM_OPTS[I8_FOLDED][1])
        c1 = _hip.conv_i8_path_counts()
        assert _form_of(fol[2]) == I8_FOLDED and fol[2].rung == rung, fol[2]
        assert (c1[0] - c0[0], c1[1] - c0[1], c1[2] - c0[2]) == (ngroups, 0, 0), (what, c0, c1)
        _same(ref4, fol, (what, "four-copy vs folded", fol[2]))
        s4 = _run(x, sd, ld, what, FORM_OPTS[I8_STRIDE4][1])
        _same(s4, fol, (what, "stride-4 vs folded"))
        f64 = _run(x, sd, ld, what, FORM_OPTS[I8_FOLDED][1], out_dtype=torch.float64)
        assert torch.equal(f64[0], fol[0].double()) and torch.equal(f64[1], fol[1].double()), (what, "folded f64")
        del ref4, s4, f64
        _check_batch_independence(x, sd, ld, fol, {}, what + " (symmetric bank)")
        _int8_oracle(fol, occ, sym, lam, els[:1] + els[-1:], what + " (symmetric bank)")
    assert _hip.conv_i8_spin_timeouts() == spins0 and _hip.device_status()[0] == 0


# ----------------------------------------------------------------------------------------------------------- coverage
# Rungs a form cannot reach with any of the sizes above, and why.  The staged template of the four-copy kernel launches at
# the big tile only (conv_i8.hip, plan_four_copy: "staging only pays with the big tile"); everything else is reachable:
# the double-buffered fp32 kernel stages (TZ + kz - 1)(TX + kx - 1) <= 144 halo rows in registers, which keeps it at {4,4}
# and below at 9^3 and (9,7,7), but {4,8} fits at (9,5,5) and (6,5,6), {8,8} at (3,3,17).
UNREACHABLE = {(I8_STAGED, r) for r in RUNGS[1:]}


def test_every_reachable_rung_was_run(hip_device):
    assert CASES_RUN == {("fp32", c) for c in FP32_CASES} | {("int8", c) for c in I8_CASES}, \
        "the coverage check needs the whole module to have run"
    reachable = set()
    for form in FORMS:
        fam = 16 if form in (I8_STRIDE4, I8_FOLDED) else 4
        for rung in RUNGS:
            if any(_find(form, ks, G, rung, RAGGED[fam] + [THIN[fam]]) for ks, G in SIZES):
                reachable.add((form, rung))
    for form in FORMS:
        for rung in RUNGS:
            n = len(RAN.get((form, rung), []))
            state = f"{n} launches" if n else ("UNREACHABLE" if (form, rung) not in reachable else "NOT RUN")
            print(f"{form:22s} {rung[0]}x{rung[1]}x64: {state}" + (f", e.g. {RAN[(form, rung)][0]}" if n else ""))
    missing = sorted(reachable - set(RAN))
    assert not missing, f"reachable but never run: {missing}"
    assert {(f, r) for f in FORMS for r in RUNGS} - reachable == UNREACHABLE
