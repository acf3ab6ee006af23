"""The fp64 twin of the generator oracle (oracle/geneo_oracle.py with dtype=torch.float64) and the parameter grid built on
it (oracle/generator_grid.py): the twin is the same function as the pinned fp32 oracle, its forward-mode Jacobian is the
derivative reverse-mode autograd gives, the clamp of the v2 cone angle opens and closes where the reference's fp32 clamp
does, and the batched evaluation the GPU tests use gives the bits of a loop."""
import numpy as np
import pytest
import torch

from oracle import geneo_oracle as go
from oracle import generator_grid as gg

FIXED = {
    "cy": dict(radius=2.3, sigma=1.4), "cone": dict(radius=1.7, sigma=1.2, apex=3.0, cone_radius=2.5, cone_inc=0.21),
    "neg": dict(radius=2.6, sigma=0.8, neg_factor=0.3),
    "cy_v1": dict(radius=2.1, sigma=1.6), "cone_v1": dict(radius=1.9, sigma=1.5, apex=3.0, cone_radius=2.2, cone_inc=0.6),
    "neg_v1": dict(radius=2.4, sigma=2.5, neg_factor=0.25),
}


@pytest.mark.parametrize("kind", gg.KINDS)
@pytest.mark.parametrize("ks", gg.CORE_SIZES)
def test_twin_is_the_fp32_oracle_up_to_fp32_rounding(kind, ks):
    """fp64 form - fp32 form < 1e-6 max|f| at a well-conditioned parameter point (measured: at most 2.5e-7); the default
    path still returns fp32, and the twin fp64."""
    k32 = go.geneo_kernel(kind, ks, FIXED[kind])
    k64 = go.geneo_kernel(kind, ks, FIXED[kind], dtype=torch.float64)
    raw = go.geneo_kernel(kind, ks, FIXED[kind], dtype=torch.float64, projected=False)
    assert k32.dtype == torch.float32 and k64.dtype == torch.float64 and k64.shape == tuple(ks)
    dev = ((k64 - k32.double()).abs().max() / raw.abs().max()).item()
    print(kind, ks, "fp64 - fp32:", dev)
    assert dev < 1e-6
    bank = go.geneo_bank([(kind, FIXED[kind])], ks, dtype=torch.float64)
    assert bank.dtype == torch.float64 and torch.equal(bank[0, 0], k64)
    assert torch.equal(go.geneo_bank([(kind, FIXED[kind])], ks)[0, 0], k32.double())


@pytest.mark.parametrize("kind", gg.KINDS)
@pytest.mark.parametrize("ks", gg.CORE_SIZES)
def test_projection_switch(kind, ks):
    """projected=False is the generator before the mean subtraction and the neg_factor constant: projecting it by hand
    gives the kernel."""
    sets = gg.core_sets(kind, ks)
    K, _ = gg.twin(kind, ks, sets, jacobian=False)
    f, _ = gg.twin(kind, ks, sets, projected=False, jacobian=False)
    vol = K.shape[1]
    if kind.startswith("neg"):
        nf = gg.widened(sets, ("neg_factor",)).double()
        want = f - f.mean(-1, keepdim=True) - (nf if kind == "neg_v1" else nf / vol)
    else:
        fz = f.reshape(len(sets), ks[0], -1)
        want = (fz - fz.mean(-1, keepdim=True)).reshape(len(sets), vol)
    scale = f.abs().amax(-1, keepdim=True) + 1.0
    assert ((K - want).abs() / scale).max().item() < 1e-14


@pytest.mark.parametrize("kind", gg.KINDS)
@pytest.mark.parametrize("ks", gg.CORE_SIZES)
def test_forward_mode_jacobian_is_reverse_mode_autograd(kind, ks):
    """<dW, J_theta> with the twin's forward-mode Jacobian == reverse-mode fp64 autograd through the twin, to 1e-12 of the
    term scale S = sum |dW_i J_theta,i|, over the whole core tier; and the reference is finite on all of it."""
    r = gg.reference(kind, ks, "core")
    for name in ("K64", "K32", "g32", "ref", "S"):
        assert torch.isfinite(r[name]).all(), name
    P = gg.widened(r["sets"], gg.SLOTS[kind]).double()
    rev = torch.empty_like(r["ref"])
    for apex, rows in gg._groups(kind, r["sets"]).items():
        f = gg._generator(kind, ks, apex, torch.float64, True)
        rev[rows] = torch.func.vmap(lambda v, d: torch.func.vjp(f, v)[1](d)[0])(P[rows], r["dW"][rows].double())
    err = (rev - r["ref"]).abs()   # (1e-290: where the terms are fp64 denormals, radius 8 beside sigma 0.3)
    assert (err <= 1e-12 * r["S"] + 1e-290).all(), float((err / r["S"].clamp_min(1e-280)).max())
    for n, s in enumerate(r["sets"]):   # what vanishes term by term in the kernels vanishes in the twin
        for j, (name, zero) in enumerate(gg.structural_zero(kind, ks, s).items()):
            if zero:
                assert r["S"][n, j].item() == 0.0, (s, name)


def test_core_tier_is_the_full_product():
    n = {kind: sum(len(gg.core_sets(kind, ks)) for ks in gg.CORE_SIZES) for kind in gg.KINDS}
    assert n == {"cy": 48, "cy_v1": 48, "neg": 192, "neg_v1": 192, "cone": 12 * 2 * 6 * 19, "cone_v1": 12 * 2 * 4 * 19}
    assert gg.apex_values(9) == [0.0, 0.9, 3.7, 8.0, 9.0] and gg.apex_values(3) == [0.0, 0.9, 3.0, 2.0]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_clamp_mask_opens_and_closes_where_the_fp32_clamp_does(dtype):
    """Open at 0.0, -0.0 and float32(0.499); closed at the fp32 neighbours outside.  (A clamp at the double 0.499 would
    close float32(0.499), which is a little larger.)"""
    below = np.nextafter(np.float32(0.0), np.float32(-1.0))
    assert float(gg.CLAMP_HI) > 0.499 and gg.CLAMP_HI_UP > gg.CLAMP_HI and below < 0
    for value, is_open in ((0.0, True), (-0.0, True), (gg.CLAMP_HI, True), (np.float32(0.25), True),
                           (below, False), (gg.CLAMP_HI_UP, False), (np.float32(-0.1), False), (np.float32(0.7), False)):
        leaf = torch.tensor(float(value), dtype=dtype, requires_grad=True)
        go.clamped_inc(leaf, dtype).backward()
        assert leaf.grad.item() == (1.0 if is_open else 0.0), (value, dtype)
    # and through the whole v2 cone, at the upper end (at inc = 0 every cone slice has rad_h = 0: no signal either way)
    for value, is_open in ((gg.CLAMP_HI, True), (gg.CLAMP_HI_UP, False)):
        leaf = torch.tensor(float(value), dtype=dtype, requires_grad=True)
        k = go.arrow_kernel((6, 5, 6), 2.3, 1.4, 2.0, 0.01, leaf, dtype=dtype)
        (k * torch.arange(k.numel(), dtype=dtype).reshape(k.shape).sin()).sum().backward()
        assert (leaf.grad.item() != 0.0) == is_open, (value, dtype, leaf.grad.item())
    # the twin's clamped angle is the fp32 one widened
    assert go.clamped_inc(0.7, torch.float64).item() == float(go.clamped_inc(0.7).item()) == float(gg.CLAMP_HI)


@pytest.mark.parametrize("kind", ["cone", "cone_v1", "neg", "neg_v1"])
def test_batched_oracle_gives_the_bits_of_a_loop(kind):
    """oracle32 (torch.func.vmap over the parameter sets) == the fp32 oracle called set by set with autograd, bit for bit,
    kernels and gradients."""
    ks = (6, 5, 6)
    sets = gg.core_sets(kind, ks)[::7]
    dW = gg.cotangents(kind, ks, len(sets), "loop")
    K, G = gg.oracle32(kind, ks, sets, dW)
    for n, s in enumerate(sets):
        leaf = {k: torch.tensor(v, dtype=torch.float32, requires_grad=(k != "apex")) for k, v in s.items()}
        k = go.geneo_kernel(kind, ks, leaf)
        assert torch.equal(k.reshape(-1), K[n]), s
        (k * dW[n].reshape(ks)).sum().backward()
        for j, name in enumerate(gg.SLOTS[kind]):
            got = leaf[name].grad   # None: the scalar is in no slice (the v2 radius at int(apex) = 0, the v1 sigma)
            assert (0.0 if got is None else got.item()) == G[n, j].item(), (s, name)


@pytest.mark.parametrize("kind", gg.KINDS)
def test_raw_term_floor_is_confined_to_the_flat_derivatives(kind):
    """gg.stiff_floor lifts the stiff tier's floor by 2^-24 Sraw in the sigma and neg_factor slots of the v2 kinds only.
    In every other slot that member would change nothing (it is below max(|fp32 oracle - twin|, 4 * 2^-24 S) at every
    set), so confining it loosens and tightens nothing -- it only keeps the member from spreading."""
    for ks in gg.CORE_SIZES:
        r = gg.reference(kind, ks, "stiff")
        base = torch.maximum((r["g32"].double() - r["ref"]).abs(), gg.FLOOR * r["S"])
        lifted = gg.stiff_floor(kind, r["S"], r["Sraw"]) > gg.FLOOR * r["S"]
        for j, name in enumerate(gg.SLOTS[kind]):
            if kind.endswith("_v1") or name not in ("sigma", "neg_factor"):
                assert not lifted[:, j].any() and (gg.F32_EPS * r["Sraw"][:, j] <= base[:, j]).all(), (ks, name)


def test_oracle_deviation_is_what_fp32_costs():
    """The yardstick of the GPU tests: 3e-8 .. 3e-6 everywhere, 3e-5 for the v1 cone (sigma_h = cone_radius sin(.) at
    cone_inc 0.05 is small, and q^2 / 2 sigma_h^2 amplifies its rounding).  A twin that drifted from the oracle, or a
    normalisation that blew up, would show here before it loosened a GPU bound."""
    for kind in gg.KINDS:
        fwd, jac = gg.oracle_deviation(kind)
        print(kind, "forward %.2e" % fwd, " ".join("%s %.2e" % (n, j) for n, j in zip(gg.SLOTS[kind], jac)))
        hi = 5e-5 if kind == "cone_v1" else 4e-6
        assert 1e-8 < fwd < hi and all(1e-8 < j < hi for j in jac), (kind, fwd, jac)
        bf, bj = gg.bounds(kind)
        assert bf <= 8 * hi and max(bj) <= 8 * hi < 2e-3
