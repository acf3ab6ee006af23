"""
ORACLE -- TEST INFRASTRUCTURE ONLY.  Not part of the product path.

The parameter grid over which the GENEO generator and its Jacobians are pinned (tests/test_oracle_generator_fp64.py on
the CPU, tests/test_gpu_generator_grid.py on the GPU), and the two CPU references every comparison there uses:

  * the fp64 twin of oracle/geneo_oracle.py (dtype=torch.float64): kernel K64, raw generator f64 and the forward-mode
    Jacobian dK/dtheta, element by element;
  * the fp32 oracle itself (the reference's own operation sequence): kernel K32 and reverse-mode <dW, dK/dtheta>.

Both are evaluated for all parameter sets of a (kind, kernel size) at once with torch.func.vmap -- bit for bit what a loop
over the sets gives (tests/test_oracle_generator_fp64.py checks that), at a hundredth of the time.

What fp32 costs the REFERENCE is the yardstick for what it may cost the kernels: `oracle_deviation(kind)` is the fp32
oracle's worst normalised deviation from the twin over the core tier, per slot and for the forward.
"""
from __future__ import annotations

import functools
import itertools
from typing import Dict, List, Sequence, Tuple

import numpy as np
import torch

from oracle import geneo_oracle as go

KINDS = ("cy", "cone", "neg", "cy_v1", "cone_v1", "neg_v1")
# trainable scalars of a kind, in the order of the Jacobian's rows (apex is an index: no gradient, arrow.py:134)
SLOTS = {"cy": ("radius", "sigma"), "cone": ("radius", "sigma", "cone_radius", "cone_inc"),
         "neg": ("radius", "sigma", "neg_factor")}
SLOTS.update({k + "_v1": v for k, v in list(SLOTS.items())})

CORE_SIZES = ((9, 9, 9), (9, 5, 5), (6, 5, 6), (3, 7, 4))
LARGE_SIZES = ((17, 17, 17), (3, 5, 17), (5, 40, 60))   # the last: 12000 elements, the builders' limit
TINY_SIZES = ((1, 1, 1), (2, 2, 2))                     # the projection cancels everything

F32_EPS = 2.0 ** -24          # half an ulp of 1.0f
FLOOR = 4 * F32_EPS           # no fp32 evaluation is asked to be closer to fp64 than this
MARGIN = 8.0                  # kernel <= MARGIN * max(oracle's own deviation, FLOOR)
# Below fp32's smallest normal number (2^-126) a term is flushed or denormal, whatever evaluates it.  Forward: a kernel
# element may be off by that much.  Jacobians: the lost factor exp(.) is multiplied by at most r^4 / a^3 (v2) or
# q^2 / sigma^3 (v1), below 1e15 on the whole grid, so 1e-20 per unit of |dW| covers it with room.
UNDERFLOW_FWD = 1e-37
UNDERFLOW_JAC = 1e-20

CLAMP_HI = np.float32(go.CLAMP_HI)                       # float32(0.499): the last cone_inc inside the clamp
CLAMP_HI_UP = np.nextafter(CLAMP_HI, np.float32(1.0))    # the first one outside


def apex_values(kz: int) -> List[float]:
    out: List[float] = []
    for a in (0.0, 0.9, min(3.7, float(kz)), float(kz - 1), float(kz)):
        if a not in out:
            out.append(a)
    return out


def _product(**axes) -> List[Dict[str, float]]:
    names = list(axes)
    return [dict(zip(names, map(float, vals))) for vals in itertools.product(*axes.values())]


def core_sets(kind: str, ks: Sequence[int]) -> List[Dict[str, float]]:
    """The trainable range: where SGD takes the parameters within an epoch.  The reference is finite on all of it."""
    axes = dict(radius=(0.3, 2.3, 8), sigma=(0.3, 1.4, 5, -1))
    if kind.startswith("neg"):
        axes.update(neg_factor=(0, 0.3, 1.5, -0.2))
    if kind.startswith("cone"):
        axes.update(cone_radius=(0.5, 2.5), apex=apex_values(ks[0]),
                    cone_inc=(-0.3, 0.05, 0.3, 0.6) if kind == "cone_v1" else (-0.1, 0, 1e-3, 0.1, 0.25, 0.4))
    return _product(**axes)


def stiff_sets(kind: str, ks: Sequence[int]) -> List[Dict[str, float]]:
    """Corners where fp32 itself is 1e-3 .. 1e-1 away from fp64 (tan(inc pi) next to the clamp, q^2 / 2 sigma^2 at a small
    sigma amplify the rounding of the inputs): compared with the fp32 oracle only.  Every stiff value meets a mild and a
    stiff partner.  v1 cone_inc = 0 is left out: sigma_h = 0 there, and the reference itself gives NaN."""
    axes = dict(radius=(0.05, 2.3, 40), sigma=(0.05, 1.4))
    if kind.startswith("neg"):
        axes.update(neg_factor=(0.3, 1.5))
    if kind.startswith("cone"):
        axes.update(cone_radius=(0.01, 2.5, 20), apex=(0.9, float(ks[0] - 1)),
                    cone_inc=(1.5, 0.3) if kind == "cone_v1" else (0.45, 0.49, CLAMP_HI, CLAMP_HI_UP, 0.7))
    return _product(**axes)


def large_sets(kind: str, ks: Sequence[int]) -> List[Dict[str, float]]:
    """Two sets of the core tier (the CPU reference's time at 12000 elements)."""
    sets = [dict(radius=2.3, sigma=1.4), dict(radius=8.0, sigma=0.3)]
    if kind.startswith("neg"):
        sets = [dict(s, neg_factor=n) for s, n in zip(sets, (0.3, -0.2))]
    if kind.startswith("cone"):
        incs = (0.3, 0.05) if kind == "cone_v1" else (0.25, 0.4)
        sets = [dict(s, cone_radius=c, apex=a, cone_inc=i)
                for s, c, a, i in zip(sets, (2.5, 0.5), (min(3.7, float(ks[0])), 0.9), incs)]
    return sets


def widened(sets: Sequence[Dict[str, float]], names: Sequence[str]) -> torch.Tensor:
    """[N, len(names)] fp32: the values the kernels are given."""
    return torch.tensor([[s[n] for n in names] for s in sets], dtype=torch.float32).reshape(len(sets), len(names))


def _groups(kind: str, sets) -> Dict[float, List[int]]:
    """apex is truncated to an index, so it is no tensor argument: one vmap per apex value."""
    groups: Dict[float, List[int]] = {}
    for i, s in enumerate(sets):
        groups.setdefault(s.get("apex"), []).append(i)
    return groups


def _generator(kind, ks, apex, dtype, projected):
    names = SLOTS[kind]

    def f(v):
        p = {n: v[i] for i, n in enumerate(names)}
        if apex is not None:
            p["apex"] = apex
        return go.geneo_kernel(kind, ks, p, dtype=dtype, projected=projected).reshape(-1)
    return f


def twin(kind: str, ks: Sequence[int], sets, projected: bool = True, jacobian: bool = True):
    """fp64 twin over `sets`: (K [N, vol], J [N, slots, vol] | None), J[n, s, i] = dK_i / dtheta_s, forward mode."""
    ks = tuple(int(k) for k in ks)
    vol, names = ks[0] * ks[1] * ks[2], SLOTS[kind]
    P = widened(sets, names).double()
    K = torch.empty((len(sets), vol), dtype=torch.float64)
    J = torch.empty((len(sets), len(names), vol), dtype=torch.float64) if jacobian else None
    for apex, rows in _groups(kind, sets).items():
        f = _generator(kind, ks, apex, torch.float64, projected)
        K[rows] = torch.func.vmap(f)(P[rows])
        if jacobian:
            J[rows] = torch.func.vmap(torch.func.jacfwd(f))(P[rows]).transpose(1, 2)
    return K, J


def oracle32(kind: str, ks: Sequence[int], sets, dW: torch.Tensor = None):
    """The fp32 oracle over `sets`: (K [N, vol] fp32, <dW_n, dK/dtheta_s> [N, slots] fp32 by reverse mode | None)."""
    ks = tuple(int(k) for k in ks)
    vol, names = ks[0] * ks[1] * ks[2], SLOTS[kind]
    P = widened(sets, names)
    K = torch.empty((len(sets), vol), dtype=torch.float32)
    G = torch.empty((len(sets), len(names)), dtype=torch.float32) if dW is not None else None
    for apex, rows in _groups(kind, sets).items():
        f = _generator(kind, ks, apex, torch.float32, True)
        K[rows] = torch.func.vmap(f)(P[rows])
        if dW is not None:
            def vjp(v, d):
                return torch.func.vjp(f, v)[1](d)[0]
            G[rows] = torch.func.vmap(vjp)(P[rows], dW[rows].reshape(len(rows), vol).float())
    return K, G


def cotangents(kind: str, ks: Sequence[int], n: int, tag: str = "") -> torch.Tensor:
    """dW ~ N(0, 1), one row per parameter set, fixed by (kind, kernel size, tag)."""
    seed = sum(ord(c) * (i + 1) for i, c in enumerate(f"{kind}{tuple(ks)}{tag}")) % (2 ** 31)
    gen = torch.Generator().manual_seed(seed)
    return torch.randn((n, ks[0] * ks[1] * ks[2]), generator=gen, dtype=torch.float32)


def contraction(J: torch.Tensor, dW: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """ref = <dW, J_s> and the term scale S = sum |dW_i J_s,i|, both [N, slots] fp64."""
    t = J * dW.double().unsqueeze(1)
    return t.sum(-1), t.abs().sum(-1)


def project(kind: str, ks: Sequence[int], dW: torch.Tensor) -> torch.Tensor:
    """P(dW) in fp64: minus the slice mean (cy, cone) or the volume mean (neg) -- the projection is symmetric, so
    <dW, P(df/dtheta)> = <P(dW), df/dtheta>, and that is the side both the kernels and autograd sum on."""
    d = dW.double().reshape(len(dW), 1 if kind.startswith("neg") else ks[0], -1)
    return (d - d.mean(-1, keepdim=True)).reshape(len(dW), -1)


def forward_excess(K: torch.Tensor, K64: torch.Tensor, fmax: torch.Tensor) -> torch.Tensor:
    """[N]: (max_i |K_i - K64_i| - UNDERFLOW_FWD)+ / max|f|  (0 where the raw generator vanishes and K is within the floor,
    inf where it vanishes and K is not)."""
    err = ((K.double() - K64).abs().amax(-1) - UNDERFLOW_FWD).clamp_min(0.0)
    return torch.where(err == 0, torch.zeros_like(err), err / fmax)


def jacobian_excess(got: torch.Tensor, ref: torch.Tensor, S: torch.Tensor, dW: torch.Tensor) -> torch.Tensor:
    """[N, slots]: (|got - ref| - UNDERFLOW_JAC sum|dW|)+ / S, with the same conventions."""
    err = ((got.double() - ref).abs() - UNDERFLOW_JAC * dW.double().abs().sum(-1, keepdim=True)).clamp_min(0.0)
    return torch.where(err == 0, torch.zeros_like(err), err / S)


@functools.lru_cache(maxsize=None)
def reference(kind: str, ks: Tuple[int, int, int], tier: str):
    """Everything a comparison at (kind, ks, tier) needs, computed once per process: dict with sets, dW, K64, fmax
    (max |raw generator| -- plus the constant of a neg kind -- [N]), ref / S ([N, slots], fp64), K32 and g32 (the fp32
    oracle's kernel and gradients); on the stiff tier Sraw ([N, slots])."""
    sets = {"core": core_sets, "stiff": stiff_sets, "large": large_sets}[tier](kind, ks)
    dW = cotangents(kind, ks, len(sets), tier)
    K64, J = twin(kind, ks, sets)
    f64, _ = twin(kind, ks, sets, projected=False, jacobian=False)
    ref, S = contraction(J, dW)
    K32, g32 = oracle32(kind, ks, sets, dW)
    Sraw = None
    if tier == "stiff":   # sum |P(dW)_i df_i/dtheta|, the raw generator's terms: what is summed where P(df/dtheta) cancels
        Sraw = (twin(kind, ks, sets, projected=False)[1] * project(kind, ks, dW).unsqueeze(1)).abs().sum(-1)
    fmax = f64.abs().amax(-1)
    if kind.startswith("neg"):
        # W = P(f) - c with c = neg_factor (v1) or neg_factor / vol (v2).  Where f is small beside c -- radius 8 with
        # sigma 0.3 leaves max|f| below 1e-10 -- W is c to all its digits and rounds like c, so the forward's scale is
        # max|f| + |c|; against max|f| alone the fp32 oracle itself is 0.96 away from the twin.
        c = widened(sets, ("neg_factor",)).double()[:, 0].abs()
        fmax = fmax + (c if kind == "neg_v1" else c / K64.shape[1])
    return dict(sets=sets, dW=dW, K64=K64, fmax=fmax, ref=ref, S=S, Sraw=Sraw, K32=K32, g32=g32)


@functools.lru_cache(maxsize=None)
def oracle_deviation(kind: str) -> Tuple[float, Tuple[float, ...]]:
    """(forward, per slot): the fp32 oracle's worst normalised deviation from the twin over the core tier."""
    fwd, jac = 0.0, torch.zeros(len(SLOTS[kind]), dtype=torch.float64)
    for ks in CORE_SIZES:
        r = reference(kind, ks, "core")
        fwd = max(fwd, float(forward_excess(r["K32"], r["K64"], r["fmax"]).max()))
        jac = torch.maximum(jac, jacobian_excess(r["g32"], r["ref"], r["S"], r["dW"]).amax(0))
    return fwd, tuple(float(j) for j in jac)


def bounds(kind: str) -> Tuple[float, Tuple[float, ...]]:
    """What a kernel may deviate from the twin, in the same normalisation: MARGIN * max(oracle's deviation, FLOOR)."""
    fwd, jac = oracle_deviation(kind)
    return MARGIN * max(fwd, FLOOR), tuple(MARGIN * max(j, FLOOR) for j in jac)


def forward_cap(fmax: torch.Tensor, own: torch.Tensor) -> torch.Tensor:
    """[N]: what test_gpu_bank.py's bounds come to per set, as a cap on the measured forward allowance.  That file holds
    kernels of magnitude up to 2 (sigma 0.5 .. 2) to a flat 2e-6 and one of magnitude 5 to 1e-5 ("sigma = 5 scales the
    absolute error"): 2e-6 flat up to magnitude 2, 2e-6 per unit of magnitude above.  One exception: a set at which the
    fp32 ORACLE itself (`own` = max|K32 - K64|) is more than an eighth of that away from the twin gets MARGIN * own --
    the v1 kinds with radius 8 have exponents q^2 / 2 sigma^2 of 5 .. 80, each carrying its own rounding into exp(.), and
    any fp32 evaluation is up to 7e-6 off there at magnitude 1, outside the box the flat 2e-6 was ever asserted in."""
    return torch.maximum(2e-6 * torch.where(fmax > 2.0, fmax, torch.ones_like(fmax)), MARGIN * own)


def stiff_floor(kind: str, S: torch.Tensor, Sraw: torch.Tensor) -> torch.Tensor:
    """[N, slots]: the stiff tier's floor of the Jacobian scale, FLOOR * S -- and in the sigma and neg_factor slots of the
    v2 kinds also F32_EPS * Sraw, Sraw = sum |P(dW)_i df_i/dtheta| over the RAW generator.  There df/dtheta is the
    gaussian E itself (times a constant), and a floor radius that is large beside the slice makes E flat: a cone slice's
    rad_h = cone_radius h tan(inc pi) is in the hundreds or thousands next to the clamp (at cone_radius 2.5 as well as 20;
    E = 1 - 1e-7 everywhere: the member lifts the floor up to 500 x), radius 40 goes part of the way (E >= 0.98 on a
    5 x 5 floor, 0.73 .. 1 on 9 x 9: up to 22 x and 4 x; the neg kind's volumes likewise, 18 x .. 2 x).  Then P(E) all
    but vanishes and S with it, while kernel and autograd alike sum the terms P(dW)_i E_i, each rounded at its own size:
    the total cancellation of the 1 x 1 x 1 and 2 x 2 x 2 sizes.  No other slot has a flat derivative, so no other slot
    gets the member."""
    floor = FLOOR * S
    if not kind.endswith("_v1"):
        for name in ("sigma", "neg_factor"):
            if name in SLOTS[kind]:
                j = SLOTS[kind].index(name)
                floor[:, j] = torch.maximum(floor[:, j], F32_EPS * Sraw[:, j])
    return floor


def structural_zero(kind: str, ks: Sequence[int], s: Dict[str, float]) -> Dict[str, bool]:
    """Slots whose gradient vanishes term by term: cone slots when no slice is a cone slice, cone_inc outside the clamp
    (v2), the v2 cone's radius and the v1 cone's sigma when no slice is a cylinder slice (the v1 cone slices have
    sigma_h = cone_radius sin(.) in sigma's place, the v2 ones rad_h in radius')."""
    out = {n: False for n in SLOTS[kind]}
    if kind.startswith("cone"):
        hc = int(np.float32(s["apex"]))
        inc = np.float32(s["cone_inc"])
        out["cone_radius"] = out["cone_inc"] = hc == int(ks[0])
        if kind == "cone":
            out["cone_inc"] |= bool(inc < 0 or inc > CLAMP_HI)
            out["radius"] = hc == 0
        else:
            out["sigma"] = hc == 0
    return out
