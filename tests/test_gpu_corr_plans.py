"""The backward correlation (sn_conv_corr_ws) on the MI355X where one workgroup runs many jobs, and at every other fork
of its three kernels that small grids never reach: csrc/corr.hip (K4 the fp32-MFMA GEMM form, K4s the gather over the set
voxels of binary occupancy) and the thread-per-tap kernel of csrc/backward.hip.

Every case asks the library's plan query (sn_conv_corr_plan) first and asserts the fork it is there for -- more jobs than
workgroups (the accumulators, K4's flag parity and the whole of K4s's software pipeline then carry over from job to job), a
second row tile, K4's every-step branch (Y > 128), the kz <= 16 instantiations, one-group and 512-group gathers, two tiles
of the fallback per axis -- and only then launches.  The shapes live in corr_plan_cases.py, where test_corr_plan_host.py
checks the same forks on any machine.

Reference: the fp64 weight gradient of a one-kernel conv3d on the CPU, with and without the relu(tanh) derivative (`out`
zero on about half the voxels); for bf16 gradients, on the rounded values.  Bars, sharpest last:

  outer   |C - want| < 2e-4 * max(1, max|want|)                          (test_gpu_backward.py's)
  inner   |C - want|[t] <= A * sqrt(N_t) * 2^-24 * S_t + 1e-30           per tap t
          S_t the same reference call on |x| and |delta|, N_t on (x != 0) and (delta != 0): the terms of tap t
  exact   x with one set voxel (or gout with one non-zero element) and out = None: every tap is one element of gout (one
          gout * x product with x in {0, 1}) or 0; adding zeros is exact, so torch.equal with the tensor gathered on the CPU.
          These pin single taps at grid corners, at the seam of two row tiles (rows taken from the plan), in the last y
          column and in the last batch element of a many-jobs case.
  bits    two runs of every launch give the same bits; a pointer that breaks the vector staging changes how a tile is
          loaded, never the order of a sum, so misaligned == aligned bit for bit; bf16 == the same values widened.

A was measured on a CPU, not on the kernel (tools/corr_bar_constant.py): the operation emulated in fp32 -- delta formed
in fp32 (gout * (1 - out * out), each operation rounded), one fp32 accumulator per partial row (a (b, z) delta plane, terms
in memory order), rows then added in fp32 -- against fp64, for every grid, kernel size and density compared below, on 8
seeds; largest |emu - ref| / (sqrt(N_t) 2^-24 S_t) over all taps, without ("plain") and with the derivative:

    grid          kernel     density  plain   deriv. | grid          kernel     density  plain   deriv.
    2x50x8x8      (3,3,3)    0.03     0.195    0.150 | 1x12x10x16    (11,3,5)   0.05     0.166    0.326
    2x50x8x8      (3,3,3)    0.6      0.005    0.013 | 1x12x10x16    (11,3,5)   0.5      0.025    0.047
    2x50x8x8      (3,3,3)    layered  0.108    0.124 | 1x20x9x12     (16,5,4)   0.05     0.213    0.308
    3x40x9x12     (5,3,5)    0.03     0.067    0.109 | 1x20x9x12     (16,5,4)   0.5      0.025    0.047
    3x40x9x12     (5,3,5)    0.6      0.003    0.009 | 1x5x12x16     (1,1,1)    0.05     0.091    0.199
    3x40x9x12     (5,3,5)    layered  0.064    0.093 | 1x5x12x16     (1,1,1)    0.5      0.027    0.016
    7x40x10x20    (9,9,9)    0.03     0.050    0.091 | 1x5x12x16     (3,16,16)  0.05     0.804   16.438
    7x40x10x20    (9,9,9)    0.6      0.002    0.006 | 1x5x12x16     (3,16,16)  0.5      0.099    0.212
    7x40x10x20    (9,9,9)    layered  0.026    0.047 | 1x5x12x16     (3,1,16)   0.05     0.202    0.554
    13x64x8x8     (3,3,3)    0.03     0.042    0.063 | 1x5x12x16     (3,1,16)   0.5      0.053    0.073
    13x64x8x8     (3,3,3)    0.6      0.002    0.004 | 1x5x12x16     (3,16,1)   0.05     0.243    1.291
    13x64x8x8     (3,3,3)    layered  0.015    0.037 | 1x5x12x16     (3,16,1)   0.5      0.063    0.182
    1x6x60x300    (3,3,5)    0.01     0.018    0.038 | 1x5x12x16     (3,17,17)  0.05     0.804   16.438
    1x6x60x300    (3,3,5)    0.6      0.002    0.003 | 1x5x12x16     (3,17,17)  0.5      0.099    0.251
    22x6x60x300   (3,3,5)    0.01     0.001    0.002 | 1x5x12x16     (3,20,20)  0.05     0.839   25.967
    1x6x60x132    (3,3,5)    0.01     0.030    0.070 | 1x5x12x16     (3,20,20)  0.5      0.172    0.779
    1x6x60x132    (3,3,5)    0.6      0.004    0.009 | 2x11x13x70    (3,3,17)   0.05     0.015    0.030
    1x3x9x1700    (3,3,3)    0.01     0.065    0.090 | 2x11x13x70    (3,3,17)   0.5      0.003    0.007
    1x3x9x1700    (3,3,3)    0.6      0.007    0.012 | 1x2x3x2200    (3,3,3)    0.05     0.116    0.142
    2x6x9x16      (3,5,3)    0.05     0.148    0.296 | 1x2x3x2200    (3,3,3)    0.5      0.027    0.042
    2x6x9x16      (3,5,3)    0.5      0.017    0.037 | 2x7x11x13     (5,3,5)    0.05     0.136    0.265
                                                     | 2x7x11x13     (5,3,5)    0.5      0.020    0.030

The two operations get a constant each, 4 times their largest ratio (the kernels sum in group / wave / row orders of their
own, and the maximum here runs over more taps than the emulation's):  A = 4 x 0.8385 = 3.354 without `out`, 4 x 25.967 =
103.868 with it.  The derivative's constant is that large because of the operation, not of a kernel: 1 - out * out in fp32
carries the rounding of out * out, 2^-25 out^2 / (1 - out^2) of the factor, which is unbounded as out -> 1 while S_t shrinks
with the factor; it shows on the far taps of a wide kernel over a sparse grid, which have one or two terms (a single
constant for both operations would have been 103.868 for the plain sums too).  A single wrong term still fails the
derivative's bar for every tap with fewer than ~3000 terms.  The emulation's x is binary; for the f32 / f64 / u8 inputs of
the GEMM form the rounding of the products adds at most 2^-24 S_t, less than a third of the bar at N_t = 1.

The last test checks coverage: every fork named above was launched; the forks the query shows to be unreachable are named
there."""
from typing import NamedTuple

import pytest
import torch

from scene_net_amd import _hip

import corr_plan_cases as cases

pytestmark = pytest.mark.gpu
A_PLAIN, A_DERIVATIVE = 4 * 0.8385, 4 * 25.967      # without / with `out`
DENSITIES = list(cases.MANY_JOBS_DENSITIES)
RAN = []            # one record per launch the plan query described
TESTS_RUN = set()
_REFS = {}


# ------------------------------------------------------------------------------------------------------------ data
def _occupancy(shape, density, gen):
    if density == "layered":     # all empty but two z planes at density 0.5: most jobs of a workgroup have nothing in reach
        x = torch.zeros(shape, dtype=torch.bool)
        for z in (shape[2] // 3, shape[2] - 2):
            x[:, :, z] = torch.rand((shape[0], 1) + tuple(shape[3:]), generator=gen) < 0.5
        return x
    return torch.rand(shape, generator=gen) < density


def _data(shape, density, seed, x_dtype=torch.bool, g_dtype=torch.float32):
    """x, gout, out on the CPU, as stored: out = relu(tanh(.)) is zero on about half the voxels"""
    gen = torch.Generator().manual_seed(seed)
    occ = _occupancy(shape, density, gen)
    g = torch.randn(shape, generator=gen).to(g_dtype)
    o = torch.tanh(torch.randn(shape, generator=gen)).clamp_min(0.0).to(g_dtype)
    if x_dtype == torch.bool:
        x = occ
    elif x_dtype == torch.uint8:
        x = (torch.randint(1, 256, shape, generator=gen) * occ).to(torch.uint8)
    else:   # (f64: the f32 values widened -- the kernel rounds on load, which the bar's constant does not model)
        x = (torch.randn(shape, generator=gen) * occ).to(x_dtype)
    return x, g, o


class Ref(NamedTuple):
    want: torch.Tensor     # fp64 [kz,kx,ky]
    S: torch.Tensor        # sum of |terms|
    N: torch.Tensor        # number of non-zero terms


def _weight_grad(x64, d64, ks):
    w = torch.zeros((1, 1) + tuple(ks), dtype=torch.float64, requires_grad=True)
    (torch.nn.functional.conv3d(x64, w, padding="same") * d64).sum().backward()
    return w.grad[0, 0]


def _ref(key, x, g, o, ks):
    """the fp64 reference of conv_corr(x, g, o, ks) on the values as stored; computed once per key"""
    if key not in _REFS:
        x64, d = x.double(), g.double()
        if o is not None:
            o64 = o.double()
            d = d * (o64 > 0) * (1 - o64 ** 2)
        _REFS[key] = Ref(_weight_grad(x64, d, ks), _weight_grad(x64.abs(), d.abs(), ks),
                         _weight_grad((x64 != 0).double(), (d != 0).double(), ks).round())
    return _REFS[key]


# ---------------------------------------------------------------------------------------------------------- launches
def _corr(x, g, o, ks, opts, fork, what, note=True):
    """conv_corr under `opts`, twice (same bits), after the plan query confirmed the fork; -> (C, plan)"""
    with _hip.options(**opts):
        plan = _hip.conv_corr_plan(x, ks, g.dtype)
        assert not cases.fork_misses(plan, fork), (what, plan, fork)
        C = _hip.conv_corr(x, g, o, ks)
        again = _hip.conv_corr(x, g, o, ks)
    assert torch.equal(C, again), (what, "two runs differ")
    if note:
        RAN.append(dict(what=what, plan=plan, g=g.dtype, groups=512 // (ks[1] * ks[2]) if plan.kernel == "gather" else 0))
    return C, plan


def _check(C, ref, what, with_out):
    A = A_DERIVATIVE if with_out else A_PLAIN
    err = (C.cpu().double() - ref.want).abs()
    outer = 2e-4 * max(1.0, ref.want.abs().max().item())
    bar = A * ref.N.sqrt() * 2.0 ** -24 * ref.S + 1e-30
    ratio = (err / (bar / A)).max().item()
    print(f"{what}: max err {err.max().item():.3e} (outer bar {outer:.3e}), worst err / (sqrt(N) 2^-24 S) {ratio:.3f} (A {A:.3f})")
    assert err.max().item() < outer, (what, err.max().item(), outer)
    bad = err > bar
    assert not bool(bad.any()), (what, "taps over the inner bar", bad.nonzero().tolist()[:8], ratio)


def _run_case(dev, case, density, seed, what, g_dtype=torch.float32, x_dtype=torch.bool, outs=(False, True)):
    x, g, o = _data(case.shape, density, seed, x_dtype, g_dtype)
    xd, gd, od = x.to(dev), g.to(dev), o.to(dev)
    got = {}
    for with_out in outs:
        tag = f"{what}, density {density}, {'out' if with_out else 'no out'}, {g_dtype}"
        C, plan = _corr(xd, gd, od if with_out else None, case.ks, case.opts, case.fork, tag)
        _check(C, _ref((case.shape, case.ks, density, seed, x_dtype, g_dtype, with_out), x, g, o if with_out else None,
                       case.ks), tag, with_out)
        got[with_out] = C
    return got


# ------------------------------------------------------------------------------------------- many jobs per workgroup
@pytest.mark.parametrize("density", DENSITIES, ids=str)
@pytest.mark.parametrize("name", list(cases.MANY_JOBS))
def test_many_jobs_per_workgroup(hip_device, name, density):
    """more jobs than workgroups: accumulators and K4's flag parity persist over job += gridDim.x; K4s's pipeline (lengths two
    jobs ahead, delta / output / chunk one ahead, empty jobs skipped between jobs with work -- the layered grid --, the
    multiply-high job decode) against the reference"""
    TESTS_RUN.add(("many", name, density))
    _run_case(hip_device, cases.MANY_JOBS[name], density, 11, name)


@pytest.mark.parametrize("name", list(cases.MANY_JOBS))
def test_many_jobs_both_kernels_agree_and_tile_sizes_agree(hip_device, name):
    """the same layered data through the other kernel and, for the gather, through the default tile (every workgroup one job):
    all within the bars of the same reference"""
    TESTS_RUN.add(("many_other", name))
    case = cases.MANY_JOBS[name]
    x, g, o = _data(case.shape, "layered", 11)
    ref = _ref((case.shape, case.ks, "layered", 11, torch.bool, torch.float32, True), x, g, o, case.ks)
    xd, gd, od = x.to(hip_device), g.to(hip_device), o.to(hip_device)
    for opts, kernel in ((cases.gather(0), "gather"), (cases.DENSE, "gemm")):
        C, _ = _corr(xd, gd, od, case.ks, opts, dict(kernel=kernel), f"{name} through {kernel}")
        _check(C, ref, f"{name} through {kernel}", True)


# --------------------------------------------------------------------------- K4: row tiles and the every-step branch
@pytest.mark.parametrize("name", list(cases.GEMM_TILES))
def test_gemm_row_tiles_and_every_step(hip_device, name):
    TESTS_RUN.add(("gemm_tiles", name))
    case = cases.GEMM_TILES[name]
    big = case.shape[0] > 1      # 2.4 M voxels: one density, with the derivative only
    for density in (cases.TILES_DENSITIES[:1] if big else cases.TILES_DENSITIES):
        _run_case(hip_device, case, density, 5, name, outs=(True,) if big else (False, True))


# ------------------------------------------------------------------------------------------------------- KZMAX = 16
@pytest.mark.parametrize("g_dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("kernel", ["gather", "gemm"])
@pytest.mark.parametrize("name", list(cases.KZ16))
def test_kz_up_to_16(hip_device, name, kernel, g_dtype):
    TESTS_RUN.add(("kz16", name, kernel, g_dtype))
    shape, ks = cases.KZ16[name]
    case = cases.Case(shape, ks, cases.gather(0) if kernel == "gather" else cases.DENSE, dict(kernel=kernel, kzmax=16))
    for density in cases.SMALL_DENSITIES:
        _run_case(hip_device, case, density, 7, f"{name} {kernel}", g_dtype=g_dtype)


# ---------------------------------------------------------------------------------------------------------- extents
@pytest.mark.parametrize("kernel", ["gather", "gemm"])
@pytest.mark.parametrize("ks", cases.EXTENTS_BOTH, ids=lambda k: "x".join(map(str, k)))
def test_extents_1_and_16(hip_device, ks, kernel):
    """kx = 1 (K4's ncol clamp), one tap per plane (512 gather groups, a quad of 2048 list entries), 256 taps (2 groups).
    (Regression: the list kernel once padded a list with one entry per thread -- 256 of the up to 4 x groups a quad needs,
    so for kx ky < 8 the gather walked whatever the workspace held: max error 8.8e3 at (1,1,1) here.)"""
    TESTS_RUN.add(("extent", ks, kernel))
    fork = dict(kernel="gather", kzmax=9, multi_group=True) if kernel == "gather" else dict(kernel="gemm", kzmax=9)
    case = cases.Case(cases.EXTENT_SHAPE, ks, cases.gather(0) if kernel == "gather" else cases.DENSE, fork)
    for density in cases.SMALL_DENSITIES:
        _run_case(hip_device, case, density, 3, f"extent {ks} {kernel}")


@pytest.mark.parametrize("kernel", ["gather", "taps"])
@pytest.mark.parametrize("ks", cases.EXTENTS_WIDE, ids=lambda k: "x".join(map(str, k)))
def test_extents_past_16(hip_device, ks, kernel):
    """kx ky > 256: one gather group, the threads past it walk group 0 and their sums are dropped; corr_dense = 1 must report
    and run the thread-per-tap kernel"""
    TESTS_RUN.add(("wide", ks, kernel))
    fork = dict(kernel="gather", multi_group=False) if kernel == "gather" else dict(kernel="taps", kzmax=0)
    case = cases.Case(cases.EXTENT_SHAPE, ks, cases.gather(0) if kernel == "gather" else cases.DENSE, fork)
    for density in cases.SMALL_DENSITIES:
        _run_case(hip_device, case, density, 3, f"extent {ks} {kernel}")


# ---------------------------------------------------------------------------------------------------- fallback tiling
@pytest.mark.parametrize("name", list(cases.TAPS_TILES))
def test_thread_per_tap_tiles(hip_device, name):
    TESTS_RUN.add(("taps", name))
    for density in cases.SMALL_DENSITIES:
        _run_case(hip_device, cases.TAPS_TILES[name], density, 9, name)


# --------------------------------------------------------------------------------------------------------- alignment
def _shifted(t):
    """the same values as a contiguous view one element into a larger buffer: 1 (bool, u8), 2 (bf16), 4 (f32), 8 (f64) bytes off"""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 != 0 and t.data_ptr() % 16 == 0
    return v


ALIGN_CASES = [("gather", torch.bool, torch.float32), ("gather", torch.bool, torch.bfloat16),
               ("gemm", torch.bool, torch.float32), ("gemm", torch.uint8, torch.float32), ("gemm", torch.float32, torch.float32),
               ("gemm", torch.float64, torch.float32), ("gemm", torch.bool, torch.bfloat16)]


@pytest.mark.parametrize("kernel,x_dtype,g_dtype", ALIGN_CASES,
                         ids=[f"{k}-{str(x)[6:]}-{str(g)[6:]}" for k, x, g in ALIGN_CASES])
def test_misaligned_pointers_give_the_same_bits(hip_device, kernel, x_dtype, g_dtype):
    """Y % 8 == 0 admits every vector staging form (K4 vec, K4s vec4, the list kernel's 8-byte loads); a pointer one element
    off switches them to element loads.  The tile holds the same values either way and every sum keeps its order (K4: the
    K-step marks are per column, not per load; K4s: the lists are in memory order either way), so the results are equal bit
    for bit -- x shifted alone, gout / out shifted alone.  (Regression: the gather's element staging once formed 1 - out^2
    with one fused multiply-add where its four-element staging rounded the square first, so shifted gout / out changed last
    bits of C at this very shape; both forms now call one helper, gather_delta in csrc/corr.hip.)"""
    TESTS_RUN.add(("align", kernel, x_dtype, g_dtype))
    opts = cases.gather(0) if kernel == "gather" else cases.DENSE
    fork = dict(kernel=kernel, vec=True, list_vec=True) if kernel == "gather" else dict(kernel=kernel, vec=True)
    case = cases.Case(cases.ALIGN_SHAPE, cases.ALIGN_KS, opts, fork)
    for density in cases.SMALL_DENSITIES:
        x, g, o = _data(case.shape, density, 13, x_dtype, g_dtype)
        xd, gd, od = x.to(hip_device), g.to(hip_device), o.to(hip_device)
        base = _run_case(hip_device, case, density, 13, f"aligned {kernel}", g_dtype=g_dtype, x_dtype=x_dtype)
        for with_out in (False, True):
            what = f"{kernel} {x_dtype} {g_dtype} density {density} out {with_out}"
            Cx, _ = _corr(_shifted(xd), gd, od if with_out else None, case.ks, opts, fork, what + ": x shifted", note=False)
            assert torch.equal(Cx, base[with_out]), (what, "x shifted", (Cx - base[with_out]).abs().max().item())
            Cg, _ = _corr(xd, _shifted(gd), _shifted(od) if with_out else None, case.ks, opts, fork, what + ": g shifted",
                          note=False)
            assert torch.equal(Cg, base[with_out]), (what, "gout / out shifted", (Cg - base[with_out]).abs().max().item())


# ---------------------------------------------------------------------------------------- input types, bf16 widening
@pytest.mark.parametrize("x_dtype", [torch.float32, torch.float64, torch.uint8, torch.bool], ids=lambda d: str(d)[6:])
def test_gemm_input_types_with_the_derivative(hip_device, x_dtype):
    TESTS_RUN.add(("types", x_dtype))
    case = cases.Case(cases.RAGGED_SHAPE, cases.RAGGED_KS, cases.DENSE, dict(kernel="gemm", vec=False))
    for density in cases.SMALL_DENSITIES:
        _run_case(hip_device, case, density, 17, f"ragged gemm {x_dtype}", x_dtype=x_dtype)


BF16_CASES = [("gather_9x9x9_tile20", cases.MANY_JOBS["gather_9x9x9_tile20"]), ("gemm_3x3x3", cases.MANY_JOBS["gemm_3x3x3"]),
              ("kz16_gather", cases.Case(*cases.KZ16["kz16"], cases.gather(0), dict(kernel="gather", kzmax=16))),
              ("kz16_gemm", cases.Case(*cases.KZ16["kz16"], cases.DENSE, dict(kernel="gemm", kzmax=16)))]


@pytest.mark.parametrize("name,case", BF16_CASES, ids=[n for n, _ in BF16_CASES])
def test_bf16_gradients_equal_the_same_values_widened(hip_device, name, case):
    """bf16 storage only changes the loads: products and sums are fp32 either way"""
    TESTS_RUN.add(("bf16", name))
    x, g, o = _data(case.shape, 0.3, 19, torch.bool, torch.bfloat16)
    xd, gd, od = x.to(hip_device), g.to(hip_device), o.to(hip_device)
    for out16 in (None, od):
        C16, _ = _corr(xd, gd, out16, case.ks, case.opts, case.fork, f"{name} bf16")
        C32, _ = _corr(xd, gd.float(), None if out16 is None else out16.float(), case.ks, case.opts, case.fork,
                       f"{name} widened")
        assert torch.equal(C16, C32), (name, (C16 - C32).abs().max().item())
    _check(C16, _ref((name, "bf16"), x, g, o, case.ks), f"{name} bf16", True)


# ------------------------------------------------------------------------------------------------- exact impulse tests
def _positions(shape, rows):
    """(b, z, x, y): the eight corners, both sides of the first row-tile seam, the last y column, the last batch element"""
    B, _, Z, X, Y = shape
    at = [(0, z, x, y) for z in (0, Z - 1) for x in (0, X - 1) for y in (0, Y - 1)]
    if rows < X:
        at += [(0, Z // 2, rows - 1, Y // 2), (0, Z // 2, rows, Y // 2), (B - 1, Z - 1, rows, 0), (B - 1, 0, rows - 1, Y - 1)]
    at += [(0, Z // 2, X // 2, Y - 1), (B - 1, Z // 2, X // 2, 1), (B - 1, Z - 1, X - 1, Y - 1)]
    return at


def _window(n, k, at, sign):
    """indices at + sign * (t - p) for t = 0 .. k - 1, and which of them lie in 0 .. n - 1"""
    i = at + sign * (torch.arange(k) - (k - 1) // 2)
    return i.clamp(0, n - 1), (i >= 0) & (i < n)


def _gathered(grid, at, ks, sign):
    """[kz,kx,ky]: grid[b, 0, at + sign (t - p)], zero outside the grid"""
    b, z, x, y = at
    (iz, mz), (ix, mx), (iy, my) = (_window(n, k, a, sign) for n, k, a in zip(grid.shape[2:], ks, (z, x, y)))
    vals = grid[b, 0][iz[:, None, None], ix[None, :, None], iy[None, None, :]]
    inside = mz[:, None, None] & mx[None, :, None] & my[None, None, :]
    return torch.where(inside, vals, torch.zeros((), dtype=vals.dtype))


@pytest.mark.parametrize("name", list(cases.IMPULSE))
def test_single_taps_are_exact(hip_device, name):
    """x with one set voxel u: C[t] = gout[u - t + p];  gout with one non-zero element at v: C[t] = gout[v] x[v + t - p].
    Every tap is one term plus zeros -- exact in fp32 -- so each launch must equal the gathered tensor bit for bit."""
    TESTS_RUN.add(("impulse", name))
    case = cases.IMPULSE[name]
    gen = torch.Generator().manual_seed(23)
    g = torch.randn(case.shape, generator=gen)
    xr = torch.rand(case.shape, generator=gen) < 0.4
    gd, xrd = g.to(hip_device), xr.to(hip_device)
    with _hip.options(**case.opts):
        rows = _hip.conv_corr_plan(xr, case.ks).rows
    for at in _positions(case.shape, rows):
        b, z, x, y = at
        xi = torch.zeros(case.shape, dtype=torch.bool, device=hip_device)
        xi[b, 0, z, x, y] = True
        C, _ = _corr(xi, gd, None, case.ks, case.opts, case.fork, f"{name}: x impulse at {at}")
        want = _gathered(g, at, case.ks, -1)
        assert torch.equal(C.cpu(), want), (name, "x impulse", at, (C.cpu() - want).abs().max().item())
        gi = torch.zeros(case.shape, device=hip_device)
        gi[b, 0, z, x, y] = g[b, 0, z, x, y]
        C, _ = _corr(xrd, gi, None, case.ks, case.opts, case.fork, f"{name}: gout impulse at {at}")
        want = _gathered(xr, at, case.ks, +1).float() * g[b, 0, z, x, y]
        assert torch.equal(C.cpu(), want), (name, "gout impulse", at, (C.cpu() - want).abs().max().item())


# ----------------------------------------------------------------------------------------------------------- coverage
# Forks the query shows to be unreachable:
#   the thread-per-tap kernel with bf16 gradients -- sn_conv_corr_t refuses them there (SN_ERR_UNSUPPORTED), and the plan
#   query with it (test_corr_plan_host.py);
#   K4s's four-element staging switched off by the tile's size -- the planner keeps a job's delta rows within 3072 elements,
#   the quads' limit is 4096: Y % 4 and the pointers alone decide it.
def test_every_fork_was_launched(hip_device):
    expected = {("many", n, d) for n in cases.MANY_JOBS for d in DENSITIES} | {("many_other", n) for n in cases.MANY_JOBS} \
        | {("gemm_tiles", n) for n in cases.GEMM_TILES} | {("taps", n) for n in cases.TAPS_TILES} \
        | {("kz16", n, k, g) for n in cases.KZ16 for k in ("gather", "gemm") for g in (torch.float32, torch.bfloat16)} \
        | {("extent", ks, k) for ks in cases.EXTENTS_BOTH for k in ("gather", "gemm")} \
        | {("wide", ks, k) for ks in cases.EXTENTS_WIDE for k in ("gather", "taps")} \
        | {("align",) + c for c in ALIGN_CASES} | {("bf16", n) for n, _ in BF16_CASES} \
        | {("types", d) for d in (torch.float32, torch.float64, torch.uint8, torch.bool)} \
        | {("impulse", n) for n in cases.IMPULSE}
    assert TESTS_RUN == expected, "the coverage check needs the whole module to have run"

    def meets(rec, key, want):
        return rec[key] == want if key in ("g", "groups") else not cases.fork_misses(rec["plan"], {key: want})

    def ran(**want):
        return [r for r in RAN if all(meets(r, k, v) for k, v in want.items())]

    forks = {
        "thread-per-tap kernel": dict(kernel="taps"),
        "thread-per-tap kernel, more than one x tile": dict(kernel="taps", row_tiled=True),
        "GEMM form (K4)": dict(kernel="gemm"),
        "gather (K4s)": dict(kernel="gather"),
        "K4, kz <= 9": dict(kernel="gemm", kzmax=9),
        "K4, kz <= 16": dict(kernel="gemm", kzmax=16),
        "K4s, kz <= 9": dict(kernel="gather", kzmax=9),
        "K4s, kz <= 16": dict(kernel="gather", kzmax=16),
        "K4, row tiles > 1": dict(kernel="gemm", row_tiled=True),
        "K4s, row tiles > 1": dict(kernel="gather", row_tiled=True),
        "K4, workgroups < jobs": dict(kernel="gemm", many_jobs=True),
        "K4s, workgroups < jobs": dict(kernel="gather", many_jobs=True),
        "K4, row tiles > 1 and workgroups < jobs": dict(kernel="gemm", row_tiled=True, many_jobs=True),
        "K4, every-step branch": dict(kernel="gemm", every_step=True),
        "K4, tracked steps": dict(kernel="gemm", every_step=False),
        "K4s, one group": dict(kernel="gather", groups=1),
        "K4s, 512 groups": dict(kernel="gather", groups=512),
        "K4s, 2 groups": dict(kernel="gather", groups=2),
        "K4s, list kernel without 8-byte loads": dict(kernel="gather", list_vec=False),
        "K4, f32 gradients": dict(kernel="gemm", g=torch.float32),
        "K4, bf16 gradients": dict(kernel="gemm", g=torch.bfloat16),
        "K4s, f32 gradients": dict(kernel="gather", g=torch.float32),
        "K4s, bf16 gradients": dict(kernel="gather", g=torch.bfloat16),
        "K4s, bf16 gradients and workgroups < jobs": dict(kernel="gather", g=torch.bfloat16, many_jobs=True),
        "thread-per-tap kernel, f32 gradients": dict(kernel="taps", g=torch.float32),
    }
    missing = []
    for label, want in forks.items():
        hits = ran(**want)
        print(f"{label:48s} {len(hits):4d} launches" + (f", e.g. {hits[0]['what']}: {tuple(hits[0]['plan'])}" if hits else ""))
        if not hits:
            missing.append(label)
    assert not missing, f"never launched: {missing}"
    assert not ran(kernel="taps", g=torch.bfloat16)
