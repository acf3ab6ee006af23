"""The cases of test_gpu_forward_auto.py and test_forward_auto_host.py: sn_forward_auto (csrc/conv_lin.hip), the forward a
float grid takes -- binarize_kernel classifies x on the device, then the int8 form and the fp32 form of the same forward are
both enqueued, each behind a device-side gate.

The numpy reference of the classification, in the input's own dtype:

    occ  = (v != 0).astype(uint8)
    flag = int(any(~((v == 0) | (v == 1))))

binarize_kernel's launch geometry, restated from the code (sn_forward_auto): 256 threads, thread t of the grid reads vector
t (elements 4t .. 4t + 3) and strides by the grid; blocks = min(ceil(n4 / 256) + 1, 2048) with n4 = n // 4, so a second trip
of the loop happens only for an element index of at least 2048 * 256 * 4; block 0 walks the n % 4 tail element by element.

No test lives here."""
import functools
import zlib
from typing import NamedTuple

import numpy as np
import torch

from scene_net_amd import _hip

TOL = 1e-4                      # the project's parity bar (test_gpu_conv.py: TOL)
STRIDE_ELEMENTS = 2048 * 256 * 4
BIG = (1, 1, 36, 244, 240)      # 2 108 160 elements: the smallest few planes past one trip of the grid-stride loop
GUARD_BYTES = 64                # behind occ_ws: must come back untouched
OCC_POISON, FLAG_POISON = 0xAB, -7
NP_OF = {torch.float32: np.float32, torch.float64: np.float64}
DTYPES = (torch.float32, torch.float64)
DECLINE = {"conv_i8_tolerance_ppb": 1}


# ------------------------------------------------------------------------------------------------------ classification
def odd_values(np_dtype):
    """(name, value) of the issue's table in np_dtype.  numpy: occ is 0 for the two zeros and 1 for everything else; only the
    zeros and 1.0 leave the flag down (asserted by test_forward_auto_host.py)."""
    t = np_dtype
    tiny = np.nextafter(t(0), t(1))
    assert tiny > 0 and tiny / t(2) == 0, "not the smallest subnormal"
    return [("+0", t(0.0)), ("-0", t(-0.0)), ("1", t(1.0)), ("1+ulp", np.nextafter(t(1), t(2))),
            ("1-ulp", np.nextafter(t(1), t(0))), ("subnormal", tiny), ("-subnormal", -tiny), ("0.5", t(0.5)), ("2", t(2.0)),
            ("-1", t(-1.0)), ("+inf", t(np.inf)), ("-inf", t(-np.inf)), ("nan", t(np.nan))]


def np_binarize(v):
    """(occ uint8, flag int) of a numpy array, in its own dtype"""
    v = np.asarray(v)
    with np.errstate(invalid="ignore"):
        return (v != 0).astype(np.uint8), int(np.any(~((v == 0) | (v == 1))))


def binary_grid(shape, density, seed):
    """bool numpy array"""
    return np.random.default_rng(seed).random(shape) < density


class Position(NamedTuple):
    name: str
    shape: tuple        # [B,1,Z,X,Y]
    index: int          # flat element


def positions():
    """Every position class of binarize_kernel, on the smallest grid that has it.  n = 1399 = 4 * 349 + 3: two blocks of
    vectors; the sibling grids give n % 4 = 1 and 2."""
    out = []
    body = (1, 1, 1, 1, 1399)
    n4 = 1399 // 4
    out.append(Position("element 0", body, 0))
    out.append(Position("wave 2, lane 37 of block 0", body, 4 * (2 * 64 + 37) + 2))
    out.append(Position("wave 1, lane 5 of block 1", body, 4 * (256 + 64 + 5) + 1))
    out.append(Position("last element of the vector body", body, 4 * n4 - 1))
    for n in (1397, 1398, 1399):                         # n % 4 = 1, 2, 3: every tail element
        for i in range(n // 4 * 4, n):
            out.append(Position(f"tail element {i - n // 4 * 4} of n % 4 = {n % 4}", (1, 1, 1, 1, n), i))
    for shape in ((1, 1, 11, 7, 3), (3, 1, 5, 3, 7)):    # 231 and 315: n % 4 = 3 on grids that are no single row
        n = int(np.prod(shape))
        assert n % 4 == 3
        out.append(Position(f"last tail element of {shape}", shape, n - 1))
    for n in (1, 2, 3):                                  # no vector body at all
        for i in range(n):
            out.append(Position(f"element {i} of n = {n}", (1, 1, 1, 1, n), i))
    return out


def big_positions():
    n = int(np.prod(BIG))
    assert n == 2_108_160 and n % 4 == 0 and n > STRIDE_ELEMENTS
    return [Position("first element of the second trip", BIG, STRIDE_ELEMENTS),
            Position("second trip, wave 2 lane 37", BIG, STRIDE_ELEMENTS + 4 * (2 * 64 + 37) + 3),
            Position("second trip, block 9", BIG, STRIDE_ELEMENTS + 4 * (9 * 256 + 70) + 1),
            Position("last element", BIG, n - 1),
            Position("last element of the first trip", BIG, STRIDE_ELEMENTS - 1)]


# -------------------------------------------------------------------------------------------------------------- routes
class Route(NamedTuple):
    shape: tuple
    ks: tuple
    G: int
    fused: bool         # conv_fused_supported: the linear kernel serves the shape
    bool_kernel: str    # conv_bank_plan(bool).kernel: what the byte form falls to where the linear kernel does not serve
    w24: object         # ConvFusedPlan.w24 where fused, else None


ROW1, ROW4, ROW5A, ROW5B = (2, 1, 9, 17, 68), (1, 1, 7, 7, 40), (1, 1, 5, 7, 9), (1, 1, 6, 6, 30)
ROUTES = {
    "lin24-G16": Route(ROW1, (9, 9, 9), 16, True, "four_copy", True),
    "lin32-ky12-G4": Route((1, 1, 7, 19, 40), (3, 3, 12), 4, True, "four_copy", False),
    "lin32-ky17-G2": Route((1, 1, 7, 19, 40), (3, 3, 17), 2, True, "four_copy", False),
    "lin24-G33": Route((1, 1, 9, 33, 64), (9, 9, 9), 33, True, "folded", True),
    "four-copy-G4": Route(ROW4, (3, 3, 20), 4, False, "four_copy", None),
    "four-copy-G20": Route(ROW4, (3, 3, 20), 20, False, "four_copy", None),
    "ragged-5x7x9-G4": Route(ROW5A, (3, 3, 3), 4, False, "fp32", None),
    "ragged-5x7x9-G20": Route(ROW5A, (3, 3, 3), 20, False, "fp32", None),
    "ragged-6x6x30-G4": Route(ROW5B, (3, 3, 3), 4, False, "fp32", None),
    "ragged-6x6x30-G20": Route(ROW5B, (3, 3, 3), 20, False, "fp32", None),
    # ky = 9, kz kx = 81, Y % 16 == 0 and a halo of 88 x 16 rows that the linear kernel's LDS does not hold: the only way
    # from this entry to the stride-4 kernel (see STRIDE4_QUERIES)
    "stride4-81x1x9-G3": Route((1, 1, 9, 9, 64), (81, 1, 9), 3, False, "stride4", None),
    # non-binary rows of the table: row one again at G = 4 and G = 20
    "lin24-G4": Route(ROW1, (9, 9, 9), 4, True, "four_copy", True),
    "lin24-G20": Route(ROW1, (9, 9, 9), 20, True, "four_copy", True),
}
BINARY_ROUTES = [r for r in ROUTES if r not in ("lin24-G4", "lin24-G20")]
DECLINED_ROUTES = ["lin24-G16", "four-copy-G4", "four-copy-G20"]
NONBINARY_ROUTES = ["lin24-G4", "lin24-G20", "four-copy-G4", "four-copy-G20", "ragged-5x7x9-G4", "ragged-5x7x9-G20",
                    "ragged-6x6x30-G4", "ragged-6x6x30-G20"]
# conv_fused_supported on (1,1,9,9,64): which of the four kz kx = 81 kernels the linear kernel declines
STRIDE4_QUERIES = {(27, 3, 9): True, (3, 27, 9): True, (81, 1, 9): False, (1, 81, 9): True}
# logspace exponents of the bank's kernel scales, tried in order until the int8 and the fp32 form differ in their bits
SPANS = ((-2.0, 0.5), (-3.0, 1.0), (-1.0, 0.3))


def route_plan(name):
    """What the library's own plan queries say of a route: (fused, kernel of the byte form, w24).  Host only."""
    r = ROUTES[name]
    xb = torch.zeros(r.shape, dtype=torch.bool)
    fused = _hip.conv_fused_supported(xb, r.ks)
    w24 = _hip.conv_fused_plan(r.shape, r.ks, r.G).w24 if fused else None
    return fused, _hip.conv_bank_plan(xb, (r.G,) + r.ks).kernel, w24


def _seed(*what):
    return zlib.crc32(repr(what).encode()) % 2 ** 31


@functools.lru_cache(maxsize=None)
def bank_of(name, span):
    """(bank f32 [G,kz,kx,ky], lam f32 [G]) of a route: uniform kernels of very different scale (test_gpu_conv.py), both signs
    among the coefficients"""
    r = ROUTES[name]
    g = torch.Generator().manual_seed(_seed("bank", r.ks, r.G))
    bank = (torch.rand((r.G,) + r.ks, generator=g) - 0.5) * torch.logspace(span[0], span[1], r.G).view(r.G, 1, 1, 1)
    lam = (torch.rand(r.G, generator=g) - 0.3) / r.G
    return bank.float().contiguous(), lam.float()


@functools.lru_cache(maxsize=None)
def grid_of(shape, kind, variant=0):
    """float32 [B,1,Z,X,Y] on the host (its f64 form is exact): 'binary' zeros and ones at density 0.3; 'half' the same with
    one 0.5; 'uniform' values in [0, 1); 'nan' binary with one NaN.  Never modified: share it."""
    g = torch.Generator().manual_seed(_seed("grid", shape, variant))
    x = (torch.rand(shape, generator=g) < 0.3).float()
    n = x.numel()
    at = int(torch.randint(0, n, (1,), generator=g))
    if kind == "half":
        x.view(-1)[at] = 0.5
    elif kind == "nan":
        x.view(-1)[at] = float("nan")
    elif kind == "uniform":
        x = torch.rand(shape, generator=g)
    else:
        assert kind == "binary"
    return x


@functools.lru_cache(maxsize=None)
def oracle_out(name, span, kind, variant=0):
    """relu(tanh(sum_g lambda_g conv3d(x, K_g))) in fp64 by the oracle, float64 [B,1,Z,X,Y]; computed once per case"""
    from oracle import geneo_oracle as go
    r = ROUTES[name]
    bank, lam = bank_of(name, span)
    x = grid_of(r.shape, kind, variant).double()
    act = go.conv_bank(x, bank.double().unsqueeze(1))
    return torch.relu(torch.tanh((lam.double().view(1, r.G, 1, 1, 1) * act).sum(1, keepdim=True)))
