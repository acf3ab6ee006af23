"""The cases of test_gpu_conv_lin_walk.py and test_lin_model_host.py: K3L (csrc/conv_lin.hip, sn_conv_fused) where one
workgroup walks several tiles, and a CPU model of its pre-activation that is exact.

model_pre restates the kernel operation for operation (conv_lin_tables.inc: lin_tables; conv_lin.hip: the epilogue):

    K*     the fp32 fma chain over the kernels of the bank, in order              a = fmaf(lambda_g, K_g, a)
    S, Q   S = 8355711 / max|K*|, Q = rint(K* S), both in fp64
    d0..2  the three balanced base-256 digits of Q                                Q = d0 + 256 d1 + 65536 d2
    scale  f32(f64(max|K*|) / 8355711)
    acc_d  the integer correlation of the occupancy with digit plane d, zero padding (k - 1) // 2 left, k // 2 right
    low    int32(acc1 * 256 + acc0)
    pre    f32(acc2 * 65536 + f32(low)) -- ONE rounding of the sum, which is fmaf -- times scale, in fp32

Python has no fma here, so the inputs are drawn on a dyadic grid on which the chain needs none: bank values are multiples of
2^-10 in [-0.5, 0.5] and the coefficients multiples of 2^-10 with sum |lambda| <= 4; every product is then a multiple of
2^-20, every partial sum a multiple of 2^-20 below 2 -- 21 bits, an exact fp32 number -- and the chain evaluated in fp64 is
the chain evaluated with fmaf.  kstar_chain asserts that at every step.  Everything after K* is integer arithmetic or a
single correctly rounded fp64 / fp32 operation, which numpy has.

No test lives here."""
import functools
import zlib
from typing import NamedTuple

import numpy as np
import torch
import torch.nn.functional as F

from scene_net_amd import _hip

QMAX = 8355711.0            # 127 * (1 + 256 + 65536)
RAGGED = (20, 40, 68)       # 3 x 3 x 2 = 18 tiles of 8 x 16 x 64 per element, a multiple of no tile extent
THIN = (5, 13, 132)         # 3 tiles per element; smaller than a tile, and than the 9^3 halo, in z and x
GRIDS = {"ragged": RAGGED, "thin": THIN}
MAX_VOXELS = 2_000_000      # of one case's batch
NO24 = {"conv_lin_no24": 1}


class Size(NamedTuple):
    ks: tuple
    G: int
    opts: dict          # library options the case runs under
    plan: dict          # the fork of lin_plan / of the walk loop it is there for: ConvFusedPlan fields, worked out by hand
    thin: bool          # also run on THIN


def _fork(w24, nsteps, halo_passes):
    return dict(w24=w24, nsteps=nsteps, deferred=nsteps >= 16, halo_passes=halo_passes)


# nsteps: ceil(3 kz kx / 8) at 24 bytes (ky <= 9), ceil(kz kx / 2) at 32; halo passes: ceil((8 + kz - 1)(16 + kx - 1) / 25)
SIZES = {
    "9x9x9": Size((9, 9, 9), 16, {}, _fork(True, 31, 16), True),               # w24, odd step count, deferred
    "9x9x9-no24": Size((9, 9, 9), 16, NO24, _fork(False, 41, 16), False),      # 32-byte packing, deferred
    "9x5x5": Size((9, 5, 5), 3, {}, _fork(True, 17, 13), True),                # deferral just on
    "9x7x7": Size((9, 7, 7), 5, {}, _fork(True, 24, 15), False),               # w24, even step count, deferred
    "6x5x6": Size((6, 5, 6), 5, {}, _fork(True, 12, 11), True),                # even extents; not deferred
    "5x7x3": Size((5, 7, 3), 7, {}, _fork(True, 14, 11), False),               # not deferred
    "3x3x12": Size((3, 3, 12), 4, {}, _fork(False, 5, 8), False),              # 32-byte packing (ky > 9), 5 steps
    "3x3x17": Size((3, 3, 17), 2, {}, _fork(False, 5, 8), False),              # the widest window
    "11x9x5": Size((11, 9, 5), 33, {}, _fork(True, 38, 18), True),             # 432 halo rows: remainder pass; three load loops
    "17x3x3": Size((17, 3, 3), 17, {}, _fork(True, 20, 18), False),            # remainder pass, tall kernel
    "9x11x3": Size((9, 11, 3), 3, {}, _fork(True, 38, 17), False),             # 416 halo rows
    "1x1x1": Size((1, 1, 1), 1, {}, _fork(True, 1, 6), False),                 # kx == 1, one step
}
WALK_CASES = [(name, "ragged") for name in SIZES] + [(name, "thin") for name, s in SIZES.items() if s.thin]

# what the coverage test of test_gpu_conv_lin_walk.py wants run at two or more tiles per workgroup: name -> predicate of a
# (ConvFusedPlan, kernel size) pair
FORKS = {
    "w24 deferred, odd nsteps": lambda p, ks: p.w24 and p.deferred and p.nsteps % 2 == 1,
    "w24 deferred, even nsteps": lambda p, ks: p.w24 and p.deferred and p.nsteps % 2 == 0,
    "w24 not deferred": lambda p, ks: p.w24 and not p.deferred,
    "wide deferred": lambda p, ks: not p.w24 and p.deferred,
    "wide not deferred": lambda p, ks: not p.w24 and not p.deferred,
    "halo passes > 16 under w24": lambda p, ks: p.w24 and p.halo_passes > 16,
    "kx == 1": lambda p, ks: ks[1] == 1,
}


def plan_of(size, B, grid):
    with _hip.options(**size.opts):
        return _hip.conv_fused_plan((B, 1) + tuple(grid), size.ks, size.G)


def plan_misses(plan, fork):
    return {k: (getattr(plan, k), v) for k, v in fork.items() if getattr(plan, k) != v}


def walk_batch(size, grid):
    """The smallest B with ntiles >= 2.5 x workgroups on the device at hand (256 compute units without one): every workgroup
    walks two tiles, some three, and -- workgroups being no multiple of an element's tiles -- a workgroup's consecutive tiles
    sit at different positions of their elements."""
    per_element = plan_of(size, 1, grid).ntiles
    for B in range(1, MAX_VOXELS // (grid[0] * grid[1] * grid[2]) + 1):
        p = plan_of(size, B, grid)
        if 2 * p.ntiles >= 5 * p.workgroups:
            assert p.tiles_per_workgroup_min >= 2 and p.tiles_per_workgroup_max >= 3, p
            assert p.workgroups % per_element != 0, (p, per_element)
            return B, p
    raise AssertionError(f"no batch of {grid} under {MAX_VOXELS} voxels gives 2.5 tiles per workgroup")


def occupancy(B, grid, gen):
    """bool [B,1,Z,X,Y]: element 0 at density 0.3, element 1 completely full, element 2 empty, the last element (B > 3) at
    0.03 plus two "ground" z planes at 0.25, the rest at 0.3"""
    x = torch.rand((B, 1) + tuple(grid), generator=gen) < 0.3
    if B > 1:
        x[1] = True
    if B > 2:
        x[2] = False
    if B > 3:
        u = torch.rand((1,) + tuple(grid), generator=gen)
        x[B - 1] = u < 0.03
        x[B - 1, :, :2] = u[:, :2] < 0.25
    return x


# ---------------------------------------------------------------------------------------------------------- the model
def kstar_chain(bank, lam):
    """K* [kz,kx,ky] float32: a = fmaf(lambda_g, K_g, a) over g in order, evaluated in fp64 -- exact on the dyadic grid, and
    asserted to be: every partial sum is an fp32 number, so fmaf's one rounding rounds nothing."""
    G = bank.shape[0]
    b = bank.double().numpy().reshape(G, -1)
    l = lam.double().numpy()
    assert np.array_equal(b, np.rint(b * 1024) / 1024) and np.abs(b).max() <= 0.5, "bank off the dyadic grid"
    assert np.array_equal(l, np.rint(l * 1024) / 1024) and np.abs(l).sum() <= 4.0, "coefficients off the dyadic grid"
    a = np.zeros(b.shape[1], dtype=np.float64)
    for g in range(G):
        a = l[g] * b[g] + a
        assert np.array_equal(a, a.astype(np.float32).astype(np.float64)), f"the fma chain rounds at kernel {g}"
    return a.astype(np.float32).reshape(tuple(bank.shape[1:]))


class Tables(NamedTuple):
    kstar: np.ndarray    # float32 [kz,kx,ky]
    Q: np.ndarray        # int64
    digits: np.ndarray   # int64 [3,kz,kx,ky]
    scale: np.float32


def tables(bank, lam):
    kstar = kstar_chain(bank, lam)
    m = np.float64(np.abs(kstar).max())
    assert m > 0
    S = QMAX / m
    Q = np.rint(kstar.astype(np.float64) * S).astype(np.int64)
    d0 = ((Q + 128) & 255) - 128
    q1 = (Q - d0) >> 8
    d1 = ((q1 + 128) & 255) - 128
    d2 = (q1 - d1) >> 8
    return Tables(kstar, Q, np.stack([d0, d1, d2]), np.float32(m / QMAX))


def digit_sums(x, digits):
    """acc_d [n,3,Z,X,Y] int64: the three integer correlations, 'same' padding ((k - 1) // 2 left, k // 2 right).  Run in
    fp32, where they are exact: every partial sum is an integer of magnitude <= 128 x taps < 2^24."""
    assert 128 * digits[0].size < 2 ** 24
    w = torch.from_numpy(digits.astype(np.float32)).unsqueeze(1)
    acc = F.conv3d(x.float(), w, padding="same")
    assert torch.equal(acc, acc.round())
    return acc.to(torch.int64).numpy()


def model_pre(x, bank, lam):
    """The kernel's pre-activation of x (bool [n,1,Z,X,Y]) as float32 [n,1,Z,X,Y], with the tables and the largest |low|."""
    t = tables(bank, lam)
    acc = digit_sums(x, t.digits)
    low = acc[:, 1] * 256 + acc[:, 0]
    low_max = int(np.abs(low).max())
    assert low_max < 2 ** 31
    hi = acc[:, 2].astype(np.float64) * 65536.0                                 # exact
    pre = (hi + low.astype(np.float32).astype(np.float64)).astype(np.float32)    # an integer below 2^53: one rounding, to fp32
    pre = pre * t.scale                                                          # fp32
    assert pre.dtype == np.float32
    return pre[:, None], t, low_max


def reference_pre(x, bank, lam):
    """sum_g lambda_g conv3d(x, K_g) in fp64 by the oracle: [n,1,Z,X,Y] float64"""
    from oracle import geneo_oracle as go
    G = bank.shape[0]
    act = go.conv_bank(x.double(), bank.double().unsqueeze(1))
    return (lam.double().view(1, G, 1, 1, 1) * act).sum(1, keepdim=True).numpy()


# ---------------------------------------------------------------------------------------------------------- the cases
class Case(NamedTuple):
    name: str
    size: Size
    grid: tuple
    B: int
    x: torch.Tensor       # bool [B,1,Z,X,Y]
    bank: torch.Tensor    # float32 [G,kz,kx,ky]
    lam: torch.Tensor     # float32 [G]


@functools.lru_cache(maxsize=None)
def build(name, grid_name, B):
    """Occupancy, bank and coefficients of a case.  The bank is uniform on the grid with its largest tap moved to the end
    of the range; the coefficients have both signs (G > 1) and are scaled, then put on the grid, so that the pre-activations
    of element 0 reach 1.5 or so, their largest on the positive side (where relu(tanh) is not constant)."""
    size, grid = SIZES[name], GRIDS[grid_name]
    assert B * grid[0] * grid[1] * grid[2] <= MAX_VOXELS
    gen = torch.Generator().manual_seed(zlib.crc32(f"{name}-{grid_name}".encode()) % 2 ** 31)
    x = occupancy(B, grid, gen)
    G, ks = size.G, size.ks
    ib = torch.randint(-512, 513, (G,) + ks, generator=gen)
    flat = ib.view(-1)
    top = int(flat.abs().argmax())
    flat[top] = 512 if flat[top] >= 0 else -512
    bank = (ib.double() / 1024).float()
    raw = torch.rand(G, generator=gen, dtype=torch.float64) - 0.3 if G > 1 else torch.ones(1, dtype=torch.float64)
    kraw = (raw.view(G, 1, 1, 1) * bank.double()).sum(0)
    pre = F.conv3d(x[:1].double(), kraw[None, None], padding="same")
    hi, lo = pre.max().item(), pre.min().item()
    c = 1.5 / max(hi, -lo) * (1.0 if hi >= -lo else -1.0)
    lam = (torch.round(c * raw * 1024) / 1024).float()
    return Case(f"{name}-{grid_name}", size, grid, B, x, bank, lam)


class Checked(NamedTuple):
    elements: tuple
    pre: np.ndarray       # float32 [n,1,Z,X,Y]: the model
    ref: np.ndarray       # float64 [n,1,Z,X,Y]: the oracle
    tables: Tables
    low_max: int


@functools.lru_cache(maxsize=None)
def checked(name, grid_name, B, elements):
    """Model and oracle on `elements` of a case; asserts what the case was built for: element 0 (which must come first) keeps
    the pre-activations out of saturation, 0.5 <= max|pre| <= 3, and has both signs (one tap has one: 0 or K*)."""
    case = build(name, grid_name, B)
    assert elements[0] == 0
    xs = case.x[list(elements)]
    pre, t, low_max = model_pre(xs, case.bank, case.lam)
    p0 = pre[0]
    assert 0.5 <= np.abs(p0).max() <= 3.0, (case.name, np.abs(p0).max())
    assert p0.max() > 0 and (p0.min() < 0 or t.kstar.size == 1), (case.name, p0.min(), p0.max())
    return Checked(tuple(elements), pre, reference_pre(xs, case.bank, case.lam), t, low_max)
