"""The GENEO generator (geneo_bank_body: sn_geneo_bank, sn_geneo_bank_prep) and its Jacobians (geneo_bank_bwd_kernel:
sn_geneo_bank_bwd, sn_geneo_backward) on the MI355X, against the fp64 twin of the oracle over the trainable range
(oracle/generator_grid.py): every apex split, the cone angle on, inside and past its clamp, small and negative sigma, all six
kinds, cubic and scrambled kernel sizes up to the 12000-element limit.  All parameter sets of a test are the rows of ONE
launch, so every comparison is a multi-G comparison too.

Measures.  Forward: |K_gpu - K_twin| / max|f| (f the raw generator; plus the constant of a neg kind).  Jacobian slot theta:
|got - <dW, J_theta>| / S with S = sum |dW_i J_theta,i| and J the twin's forward-mode Jacobian.  The bound is not chosen: it
is 8 x max(the fp32 ORACLE's own worst deviation from the twin in the same measure over the core tier, 4 * 2^-24), per kind
and slot -- the kernels draw other roundings of the same sums (wave shuffles against torch's pairwise order, another libm),
not other sums.  DESIGN.md ("Generator parity over the trainable range") has the table of both.  On the stiff tier fp32
itself is 1e-3 .. 1e-1 away from fp64, so there the kernel is held to the fp32 oracle, within 8 x the oracle's own distance
from the twin.  The Jacobians also meet the 2e-3 / 2e-4 of test_gpu_backward.py (against the fp32 oracle's autograd, as
there).  The forward allowance is capped by what test_gpu_bank.py asks (gg.forward_cap): a flat 2e-6 up to magnitude 2,
2e-6 per unit of magnitude above (that file's 1e-5 at sigma 5) -- but for the sets at which the fp32 oracle itself is
more than an eighth of that away from the twin, which get 8 x the oracle's distance; the test prints how many."""
import ctypes

import numpy as np
import pytest
import torch

from scene_net_amd import _hip
from scene_net_amd.geneos import KIND_OF_CLASS
from oracle import generator_grid as gg

pytestmark = pytest.mark.gpu

SN_ERR_UNSUPPORTED = -2   # include/scenenet_hip.h
COL = {"radius": _hip.SN_P_RADIUS, "sigma": _hip.SN_P_SIGMA, "apex": _hip.SN_P_APEX,
       "cone_radius": _hip.SN_P_CONE_RADIUS, "cone_inc": _hip.SN_P_CONE_INC, "neg_factor": _hip.SN_P_NEG_FACTOR}


def _pack(kind, sets, dev):
    """[N, SN_NPARAM] fp32 rows as pack_params lays them out (unused slots 0), and the kind column."""
    P = torch.zeros((len(sets), _hip.SN_NPARAM), dtype=torch.float32)
    for name, col in COL.items():
        if name in sets[0]:
            P[:, col] = torch.tensor([s[name] for s in sets], dtype=torch.float32)
    kinds = torch.full((len(sets),), KIND_OF_CLASS[kind], dtype=torch.int32)
    return P.to(dev).contiguous(), kinds.to(dev)


def _prepared_bank(P, kinds, status):
    """sn_geneo_bank_prep without coefficients, through the C ABI: _hip.geneo_bank_prep hands it no status word."""
    G = P.shape[0]
    bank = torch.full((G, 9, 9, 9), float("nan"), device=P.device)
    prep = torch.empty(_hip.SN_CONV_PREP_BYTES * ((G + 15) // 16), dtype=torch.uint8, device=P.device)
    p = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    rc = _hip.load().sn_geneo_bank_prep(p(P), p(kinds), G, 9, 9, 9, p(bank), p(status), None, None, 0, None, p(prep),
                                        _hip._stream())
    assert rc == 0, _hip.load().sn_last_error()
    return bank


def _launch(kind, ks, r, dev, prep=False):
    """One forward launch (sn_geneo_bank, or sn_geneo_bank_prep with prep=True) and one backward launch over all rows of a
    reference -> (K [N, vol], the forward launch's status [N], dparams [N, 8]), CPU."""
    P, kinds = _pack(kind, r["sets"], dev)
    N = len(r["sets"])
    status = torch.full((N,), -7, dtype=torch.int32, device=dev)
    bank = _prepared_bank(P, kinds, status) if prep else _hip.geneo_bank(P, kinds, ks, status)
    dparams = _hip.geneo_bank_bwd(P, kinds, ks, r["dW"].reshape((N,) + tuple(ks)).to(dev).contiguous())
    return bank.reshape(N, -1).cpu(), status.cpu(), dparams.cpu()


def _old_jacobian_bound_holds(got, want):
    """test_gpu_backward.py's _close, against the fp32 oracle's autograd as there."""
    got, want = got.double(), want.double()
    return (got - want).abs() <= 2e-4 + 2e-3 * torch.maximum(got.abs(), want.abs())


def _check_against_twin(kind, ks, r, K, status, dparams):
    bf, bj = gg.bounds(kind)
    of, oj = gg.oracle_deviation(kind)
    assert (status == 0).all()
    assert torch.isfinite(K).all() and torch.isfinite(dparams).all()
    fwd = gg.forward_excess(K, r["K64"], r["fmax"])
    print(f"{kind} {tuple(ks)} forward: kernel {fwd.max():.3e}  oracle {of:.3e}  bound {bf:.3e}")
    own = (r["K32"].double() - r["K64"]).abs().amax(-1)
    cap = gg.forward_cap(r["fmax"], own)
    measured = bf * r["fmax"]
    allowed = torch.minimum(measured, cap)
    print(f"{kind} {tuple(ks)} forward allowance: {len(own)} sets, the cap governs {int((cap < measured).sum())}, "
          f"scaled above magnitude 2 at {int(((cap < measured) & (r['fmax'] > 2.0)).sum())}, "
          f"lifted to 8 x oracle at {int(((cap < measured) & (cap > 2e-6 * r['fmax'].clamp_min(1.0))).sum())}, "
          f"above a flat 2e-6 at {int((allowed > 2e-6).sum())}")
    err = ((K.double() - r["K64"]).abs().amax(-1) - gg.UNDERFLOW_FWD).clamp_min(0.0)
    n = int((err - allowed).argmax())
    assert (err <= allowed).all(), (kind, ks, r["sets"][n], err[n].item(), allowed[n].item(), r["fmax"][n].item())
    cols = [COL[n] for n in gg.SLOTS[kind]]
    got = dparams[:, cols]
    jac = gg.jacobian_excess(got, r["ref"], r["S"], r["dW"])
    for j, name in enumerate(gg.SLOTS[kind]):
        print(f"{kind} {tuple(ks)} {name}: kernel {jac[:, j].max():.3e}  oracle {oj[j]:.3e}  bound {bj[j]:.3e}")
    for j, name in enumerate(gg.SLOTS[kind]):
        n = int(jac[:, j].argmax())
        assert jac[n, j].item() <= bj[j], (kind, ks, name, r["sets"][n], jac[n, j].item(), bj[j])
    assert _old_jacobian_bound_holds(got, r["g32"]).all()
    _check_zeros(kind, ks, r["sets"], dparams)


def _check_zeros(kind, ks, sets, dparams):
    """== 0.0 where the gradient vanishes term by term: the apex slot and the slots of other kinds always, the rest as
    structural_zero says."""
    cols = [COL[n] for n in gg.SLOTS[kind]]
    others = [c for c in range(_hip.SN_NPARAM) if c not in cols]
    assert (dparams[:, others] == 0.0).all()
    for n, s in enumerate(sets):
        for name, zero in gg.structural_zero(kind, ks, s).items():
            if zero:
                assert dparams[n, COL[name]].item() == 0.0, (kind, ks, s, name, dparams[n, COL[name]].item())


@pytest.mark.parametrize("kind", gg.KINDS)
@pytest.mark.parametrize("ks", gg.CORE_SIZES)
def test_core_tier(hip_device, kind, ks):
    r = gg.reference(kind, ks, "core")
    _check_against_twin(kind, ks, r, *_launch(kind, ks, r, hip_device))


@pytest.mark.parametrize("kind", gg.KINDS)
@pytest.mark.parametrize("ks", gg.LARGE_SIZES)
def test_large_sizes(hip_device, kind, ks):
    """17^3, a thin 3 x 5 x 17 and 5 x 40 x 60 = 12000 exactly (the limit), two sets of the core tier each, under the core
    tier's bound."""
    r = gg.reference(kind, ks, "large")
    _check_against_twin(kind, ks, r, *_launch(kind, ks, r, hip_device))


@pytest.mark.parametrize("kind", gg.KINDS)
def test_prepared_builder_at_9x9x9(hip_device, kind):
    """sn_geneo_bank_prep (kz = kx = ky = 9 compiled in, the int8 preparation as its tail) writes the same bank."""
    r = gg.reference(kind, (9, 9, 9), "core")
    _check_against_twin(kind, (9, 9, 9), r, *_launch(kind, (9, 9, 9), r, hip_device, prep=True))


@pytest.mark.parametrize("kind", gg.KINDS)
@pytest.mark.parametrize("ks", gg.CORE_SIZES)
def test_stiff_tier(hip_device, kind, ks):
    """sigma 0.05, radius 0.05 and 40, cone_radius 0.01 and 20, cone_inc up to, on and past the clamp (v2) and 1.5 (v1):
    |kernel - fp32 oracle| <= 8 max(|fp32 oracle - twin|, 4 * 2^-24 of the scale), set by set and slot by slot.

    In the sigma and neg_factor slots of the v2 kinds, and nowhere else, the scale's floor has a second member, 2^-24 Sraw
    with Sraw = sum |P(dW)_i df_i/dtheta| over the RAW generator (gg.stiff_floor has the reason: a floor radius that is
    large beside the slice makes the v2 gaussian, which IS df/dsigma, flat, and P of it cancels as at 2 x 2 x 2).  Where
    nothing cancels Sraw is about S and the member is below 4 * 2^-24 S.  [measured, MI355X] without it the v2 cone's
    and the v2 neg's sigma slot stand at 1.2 .. 7.2 x the allowance at such sets; every other slot of every kind is
    below 0.4 x."""
    r = gg.reference(kind, ks, "stiff")
    for name in ("K64", "K32", "g32", "ref", "S"):
        assert torch.isfinite(r[name]).all(), name
    K, status, dparams = _launch(kind, ks, r, hip_device)
    assert (status == 0).all() and torch.isfinite(K).all() and torch.isfinite(dparams).all()
    own = (r["K32"].double() - r["K64"]).abs().amax(-1)
    allowed = gg.MARGIN * torch.maximum(own, gg.FLOOR * r["fmax"]) + gg.UNDERFLOW_FWD
    err = (K.double() - r["K32"].double()).abs().amax(-1)
    print(f"{kind} {tuple(ks)} forward: kernel/allowed {(err / allowed).max():.3e}")
    assert (err <= allowed).all(), (kind, ks, r["sets"][int((err / allowed).argmax())], float((err / allowed).max()))
    got = dparams[:, [COL[n] for n in gg.SLOTS[kind]]].double()
    own = (r["g32"].double() - r["ref"]).abs()
    allowed = gg.MARGIN * torch.maximum(own, gg.stiff_floor(kind, r["S"], r["Sraw"])) \
        + gg.UNDERFLOW_JAC * r["dW"].double().abs().sum(-1, keepdim=True)
    err = (got - r["g32"].double()).abs()
    for j, name in enumerate(gg.SLOTS[kind]):
        print(f"{kind} {tuple(ks)} {name}: kernel/allowed {(err[:, j] / allowed[:, j]).max():.3e}")
    worst = int((err / allowed).amax(-1).argmax())
    assert (err <= allowed).all(), (kind, ks, r["sets"][worst], (err / allowed)[worst].tolist())
    _check_zeros(kind, ks, r["sets"], dparams)


@pytest.mark.parametrize("kind", gg.KINDS)
@pytest.mark.parametrize("ks", gg.TINY_SIZES)
def test_sizes_where_the_projection_cancels_everything(hip_device, kind, ks):
    """1 x 1 x 1 and 2 x 2 x 2: every element of a slice (of the volume, neg) is at the same distance from the centre, so
    P(f) = 0 and P(df/dtheta) = 0 -- what comes out is rounding alone: finite, structural zeros exact, and
    |got - ref| <= 8 * 2^-24 sum|dW_i| max_i |df_i/dtheta| with the RAW generator's derivative (ref = 0 but for the neg
    kinds' constant, -neg_factor / vol (v2) or -neg_factor (v1), whose derivative joins max|df/dtheta|)."""
    sets = gg.core_sets(kind, ks)
    vol = ks[0] * ks[1] * ks[2]
    dW = gg.cotangents(kind, ks, len(sets), "tiny")
    K64, J = gg.twin(kind, ks, sets)
    f64, Jraw = gg.twin(kind, ks, sets, projected=False)
    ref, _ = gg.contraction(J, dW)
    r = dict(sets=sets, dW=dW)
    K, status, dparams = _launch(kind, ks, r, hip_device)
    assert (status == 0).all() and torch.isfinite(K).all() and torch.isfinite(dparams).all()
    scale = Jraw.abs().amax(-1)
    fmax = f64.abs().amax(-1)
    if kind.startswith("neg"):
        j = gg.SLOTS[kind].index("neg_factor")
        scale[:, j] += 1.0 if kind == "neg_v1" else 1.0 / vol
        c = gg.widened(sets, ("neg_factor",)).double()[:, 0].abs()
        fmax = fmax + (c if kind == "neg_v1" else c / vol)
    else:
        assert ref.abs().max().item() < 1e-12 * max(1.0, scale.max().item())   # the twin: total cancellation
    allowed = 8 * gg.F32_EPS * dW.double().abs().sum(-1, keepdim=True) * scale
    got = dparams[:, [COL[n] for n in gg.SLOTS[kind]]].double()
    err = (got - ref).abs()
    print(f"{kind} {tuple(ks)}: worst |got - ref| / allowed {(err / allowed.clamp_min(1e-300)).max():.3e}")
    assert (err <= allowed).all(), (kind, ks, sets[int((err - allowed).amax(-1).argmax())])
    assert ((K.double() - K64).abs().amax(-1) <= 8 * gg.F32_EPS * fmax).all()
    _check_zeros(kind, ks, sets, dparams)


def _mixed_rows(ks, G, seed):
    """G rows of all six kinds in a shuffled order, parameter sets spread over the core tier."""
    rng = np.random.default_rng(seed)
    rows = []
    for i in range(G):
        kind = gg.KINDS[i % len(gg.KINDS)]
        sets = gg.core_sets(kind, ks)
        rows.append((kind, sets[int(rng.integers(len(sets)))]))
    return [rows[i] for i in rng.permutation(G)]


def _pack_mixed(rows, dev):
    parts = [_pack(kind, [s], "cpu") for kind, s in rows]
    return (torch.cat([p for p, _ in parts]).to(dev).contiguous(), torch.cat([k for _, k in parts]).to(dev))


@pytest.mark.parametrize("ks", [(9, 9, 9), (6, 5, 6)])
def test_rows_of_a_mixed_launch_equal_their_single_launches(hip_device, ks):
    """G = 33, all six kinds shuffled: row g of the bank and of the Jacobians is bit for bit what a G = 1 launch of that row
    gives (the g * vol, g * SN_NPARAM and kinds[g] indexing)."""
    G = 33
    rows = _mixed_rows(ks, G, 33)
    P, kinds = _pack_mixed(rows, hip_device)
    dW = torch.randn((G,) + tuple(ks), generator=torch.Generator().manual_seed(33)).to(hip_device).contiguous()
    status = torch.full((G,), -7, dtype=torch.int32, device=hip_device)
    bank = _hip.geneo_bank(P, kinds, ks, status)
    dparams = _hip.geneo_bank_bwd(P, kinds, ks, dW)
    assert (status == 0).all() and len({k for k, _ in rows}) == 6
    for g in range(G):
        one = _hip.geneo_bank(P[g:g + 1].contiguous(), kinds[g:g + 1].contiguous(), ks)
        assert torch.equal(one[0], bank[g]), (g, rows[g])
        one = _hip.geneo_bank_bwd(P[g:g + 1].contiguous(), kinds[g:g + 1].contiguous(), ks, dW[g:g + 1].contiguous())
        assert torch.equal(one[0], dparams[g]), (g, rows[g])


@pytest.mark.parametrize("ks", [(9, 9, 9), (6, 5, 6)])
@pytest.mark.parametrize("last", [0, 7, 19])
def test_fused_backward_at_every_position_of_the_frozen_coefficient(hip_device, ks, last):
    """sn_geneo_backward, G = 20, last first, inside and at the end: the parameter block is sn_geneo_bank_bwd on lambda_g C
    bit for bit; dlam_g is <K_g - K_last, C> in fp64 within 8 * 4 * 2^-24 of S = sum |K_g C| + sum |K_last C| (an fp32 dot
    product has no oracle deviation above the floor); dlam[last] == 0.0."""
    G = 20
    rows = _mixed_rows(ks, G, 20)
    P, kinds = _pack_mixed(rows, hip_device)
    gen = torch.Generator().manual_seed(20 + last)
    lam = (torch.rand(G, generator=gen) - 0.3).to(hip_device).contiguous()
    C = torch.randn(ks, generator=gen).to(hip_device).contiguous()
    bank = _hip.geneo_bank(P, kinds, ks)
    out = torch.full((G * _hip.SN_NPARAM + G,), float("nan"), device=hip_device)
    _hip.geneo_backward(P, kinds, ks, bank, lam, C, last, out)
    dW = (lam.reshape(G, 1) * C.reshape(1, -1)).reshape(bank.shape).contiguous()
    parts = _hip.geneo_bank_bwd(P, kinds, ks, dW)
    assert torch.equal(out[: G * _hip.SN_NPARAM].view(G, _hip.SN_NPARAM), parts)
    terms = bank.reshape(G, -1).double().cpu() * C.reshape(1, -1).double().cpu()
    want = terms.sum(-1) - terms[last].sum()
    S = terms.abs().sum(-1) + terms[last].abs().sum()
    got = out[G * _hip.SN_NPARAM:].double().cpu()
    err = (got - want).abs()
    print(f"dlam {tuple(ks)} last={last}: worst |got - ref| / S {(err / S.clamp_min(1e-300)).max():.3e}"
          f"  bound {gg.MARGIN * gg.FLOOR:.3e}")
    assert got[last].item() == 0.0
    assert (err <= gg.MARGIN * gg.FLOOR * S).all()   # (S = 0: a neg kernel with neg_factor 0 beside itself -- then 0 == 0)


@pytest.mark.parametrize("ks", [(7, 41, 42), (1, 11, 1091)])
def test_a_volume_above_12000_is_refused_by_every_entry_point(hip_device, ks):
    """12054 and 12001 elements: SN_ERR_UNSUPPORTED from the three builders and the two backward entries, nothing written
    (5 x 40 x 60 = 12000 itself is served: test_large_sizes).  sn_geneo_bank_prep serves 9 x 9 x 9 alone and refuses
    these sizes for that, before any volume is looked at: it is here so that all five refuse, not for the limit."""
    lib = _hip.load()
    dev, G = hip_device, 2
    vol = ks[0] * ks[1] * ks[2]
    sets = gg.large_sets("cone", (9, 9, 9))
    P, kinds = _pack("cone", sets, dev)
    poison = lambda *shape: torch.full(shape, float("nan"), device=dev)   # noqa: E731
    bank, dparams, lam_out, dlam = poison(G, vol), poison(G, _hip.SN_NPARAM), poison(G), poison(G)
    status = torch.full((G,), -7, dtype=torch.int32, device=dev)
    prep = torch.full((_hip.SN_CONV_PREP_BYTES,), 0xAB, dtype=torch.uint8, device=dev)
    lam = torch.tensor([0.25, 0.5], device=dev)
    order = torch.tensor([0, 1], dtype=torch.int32, device=dev)
    dW, C = torch.randn(G, vol, device=dev), torch.randn(vol, device=dev)
    kbank = torch.randn(G, vol, device=dev)
    s = _hip._stream()
    p = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    calls = {
        "sn_geneo_bank": lambda: lib.sn_geneo_bank(p(P), p(kinds), G, *ks, p(bank), p(status), s),
        "sn_geneo_bank_lambdas": lambda: lib.sn_geneo_bank_lambdas(p(P), p(kinds), G, *ks, p(bank), p(status), p(lam),
                                                                   p(order), 1, p(lam_out), s),
        "sn_geneo_bank_prep": lambda: lib.sn_geneo_bank_prep(p(P), p(kinds), G, *ks, p(bank), p(status), p(lam), p(order),
                                                             1, p(lam_out), p(prep), s),
        "sn_geneo_bank_bwd": lambda: lib.sn_geneo_bank_bwd(p(P), p(kinds), G, *ks, p(dW), p(dparams), s),
        "sn_geneo_backward": lambda: lib.sn_geneo_backward(p(P), p(kinds), G, *ks, p(kbank), p(lam), p(C), 1, p(dparams),
                                                           p(dlam), s),
    }
    for name, call in calls.items():
        assert call() == SN_ERR_UNSUPPORTED, name
        assert lib.sn_last_error().startswith(name.encode() + b":"), (name, lib.sn_last_error())
    torch.cuda.synchronize()
    for t in (bank, dparams, lam_out, dlam):
        assert torch.isnan(t).all()
    assert (status == -7).all() and (prep == 0xAB).all()
    assert torch.equal(lam.cpu(), torch.tensor([0.25, 0.5]))   # the builders refresh lambdas[last] in place when they run
