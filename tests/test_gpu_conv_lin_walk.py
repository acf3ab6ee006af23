"""K3L (csrc/conv_lin.hip, sn_conv_fused: the module's default forward) where one workgroup walks several tiles, on the MI355X.

The kernel is persistent, grid = min(compute units, tiles), and three of its mechanisms work only from a workgroup's second
tile on: the next tile's halo travels into registers while the current tile's MFMAs run (with a synchronous remainder pass
for halos of more than 16 x 25 rows), a deferred epilogue finishes a tile's outputs between the MFMAs of the next tile
(nsteps >= 16), and one halo buffer is reused behind one barrier per tile.  Every other K3L test of the suite but the
full-size 9^3 runs gives each workgroup one tile.  Here the batch size is taken from the library's own plan query
(sn_conv_fused_plan: the smallest B with 2.5 tiles per workgroup -- every workgroup walks two, some three, and consecutive
tiles of a workgroup sit at different positions of their elements) on grids that are multiples of no tile extent
(lin_cases.py: RAGGED 20 x 40 x 68, THIN 5 x 13 x 132), for a kernel size on every fork of lin_plan and of the walk loop.
Each case first reads the guard's verdict word as 0 (K3L ran, not the fp32 route) and holds the plan to the table's, then:

a. position independence, bit for bit: ten or so elements run ALONE (B = 1: one tile per workgroup, asserted -- the path
   the other tests hold against the oracle) equal their slices of the big run.  An output voxel depends on its window, K*
   and the scale, never on which workgroup reached it second or third.
b. forms at the same shape, bit for bit: the 32-byte packing against the 24-byte one (ky <= 9), tables from
   conv_fused_prep (LDS-DMA) against tables built in the kernel, f64 output == f32.double(), bf16 output ==
   f32.to(bfloat16) (one round-to-nearest-even of the same fp32 number either way), a second call.
c. the model, elementwise, on the first, full, empty, middle and last element:

       |out - relu(tanh(f64(model_pre)))| <= A = 3 x 2^-23 (3.6e-7)

   model_pre (lin_cases.py) restates the exact integer accumulation and its fp32 recombination bit for bit, so the only
   inexact step left is relu_tanh's 1 - 2 / (exp(2v) + 1) on v_exp_f32 and v_rcp_f32.  A, with u = 2^-23: 2v is exact;
   fl(2v log2e) and v_exp_f32 give E = exp(2v) to a relative (2|v| + 1) u; fl(E + 1) and v_rcp_f32 add 1.5 u; 2 / (E + 1)
   carries these as 2E(2v + 1) / (E + 1)^2 u <= 0.79 u plus 2 / (E + 1) 1.5 u <= 1.5 u; the final subtraction adds u / 4.
   This rests on the kernel comment's "1 ulp" for both instructions.
   [measured, MI355X] the worst |out - model| over the sixteen cases: 1.365e-7 = 1.145 x 2^-23 (9x9x9-no24-ragged and
   11x9x5-thin; every case but the single tap lies between 1.05 and 1.15 x 2^-23), always at a pre-activation near 0.02,
   where 1 - 2 / (E + 1) cancels (the roundings of E + 1 and of its reciprocal are absolute: they do not shrink with the result).
   Outer bars as before: the empty element is exactly 0, |out - oracle| < 1e-4 (fp64 oracle), device status 0.
d. coverage (the module's last test): from the plans actually launched, every fork of lin_cases.FORKS, every store type
   and the prepared tables ran at two or more tiles per workgroup."""
import functools
import types

import numpy as np
import pytest
import torch

from scene_net_amd import _hip

import lin_cases as lc

pytestmark = pytest.mark.gpu
TOL = 1e-4
A_BAR = 3 * 2.0 ** -23
RAN = []             # (what, ConvFusedPlan, kernel size, out dtype, prepared tables) of every launch
CASES_RUN = set()
IDS = [f"{n}-{g}" for n, g in lc.WALK_CASES]


def _launch(what, size, x, bank, lam, opts=None, **kw):
    """conv_fused under the case's options (or `opts`); what the plan query says was launched goes into the coverage table"""
    opts = size.opts if opts is None else opts
    with _hip.options(**opts):
        plan = _hip.conv_fused_plan(x, size.ks, size.G)
        out = _hip.conv_fused(x, bank, lam, **kw)
    RAN.append((what, plan, size.ks, kw.get("out_dtype", torch.float32), kw.get("prep") is not None))
    return out, plan


@functools.lru_cache(maxsize=None)
def _big(name, gname, dev):
    """the walked run of a case, once: the batch from the plan query, the guard's verdict read as 0, the plan the table's"""
    size, grid = lc.SIZES[name], lc.GRIDS[gname]
    r = types.SimpleNamespace()
    r.what = f"{name}-{gname}"
    r.size = size
    r.B, want = lc.walk_batch(size, grid)
    r.case = lc.build(name, gname, r.B)
    assert r.case.x.numel() <= lc.MAX_VOXELS
    r.x, r.bank, r.lam = r.case.x.to(dev), r.case.bank.to(dev).contiguous(), r.case.lam.to(dev)
    verdict = torch.full((1,), -1, dtype=torch.int32, device=dev)
    r.out, r.plan = _launch(r.what, size, r.x, r.bank, r.lam, verdict=verdict)
    assert verdict.item() == 0, (r.what, "the guard sent the launch to the fp32 route", verdict.item())
    assert r.plan == want and not lc.plan_misses(r.plan, size.plan), (r.what, r.plan)
    assert r.plan.tiles_per_workgroup_min >= 2 and r.plan.tiles_per_workgroup_max >= 3, (r.what, r.plan)
    return r


def _alone(B):
    """eight elements across the batch, and always the full and the empty one"""
    return sorted(set(np.linspace(0, B - 1, 8).round().astype(int).tolist()) | {1, 2})


def _first_difference(a, b):
    bad = (a != b).nonzero()
    return (len(bad), bad[0].tolist(), a[tuple(bad[0])].item(), b[tuple(bad[0])].item()) if len(bad) else None


@pytest.mark.parametrize("name,gname", lc.WALK_CASES, ids=IDS)
def test_walked_tiles_equal_the_elements_run_alone(hip_device, name, gname):
    """a. bit for bit"""
    r = _big(name, gname, str(hip_device))
    CASES_RUN.add(("alone", name, gname))
    for b in _alone(r.B):
        one, p1 = _launch(r.what + " (alone)", r.size, r.x[b:b + 1].clone(), r.bank, r.lam)
        assert p1.tiles_per_workgroup_max == 1 and p1.workgroups == p1.ntiles, (r.what, p1)
        assert torch.equal(one[0], r.out[b]), (r.what, "element", b, r.plan, _first_difference(one[0], r.out[b]))


@pytest.mark.parametrize("name,gname", lc.WALK_CASES, ids=IDS)
def test_walked_forms_agree_bit_for_bit(hip_device, name, gname):
    """b. the other packing, prepared tables, f64 and bf16 stores, a second call"""
    r = _big(name, gname, str(hip_device))
    CASES_RUN.add(("forms", name, gname))
    size = r.size
    other = {} if size.opts else lc.NO24
    with _hip.options(**other):
        has_other = _hip.conv_fused_supported(r.x, size.ks)
    # 99 kernel rows at 32 bytes are 50 steps: tables of 153 KiB and the halo do not fit the 160 KiB of LDS, no such form
    assert has_other == (size.ks[0] * size.ks[1] < 99), (r.what, has_other)
    if size.ks[2] <= 9 and has_other:
        o2, p2 = _launch(r.what + " (other packing)", size, r.x, r.bank, r.lam, opts=other)
        assert p2.w24 != r.plan.w24 and p2.ntiles == r.plan.ntiles, (r.what, p2)
        assert torch.equal(o2, r.out), (r.what, "24- vs 32-byte packing", _first_difference(o2, r.out))
        del o2
    else:
        assert not r.plan.w24 or not has_other
    with _hip.options(**size.opts):
        blob = _hip.conv_fused_prep(r.bank, r.lam)
        assert _hip.conv_fused_prep_verdict(blob, size.ks).item() == 0, (r.what, "the blob's verdict")
    for served in (False, True):
        o3, _ = _launch(r.what + " (prepared)", size, r.x, r.bank, r.lam, prep=blob, assume_served=served)
        assert torch.equal(o3, r.out), (r.what, "prepared tables, assume_served =", served, _first_difference(o3, r.out))
        del o3
    o64, _ = _launch(r.what + " (f64)", size, r.x, r.bank, r.lam, out_dtype=torch.float64)
    assert torch.equal(o64, r.out.double()), (r.what, "f64 output", _first_difference(o64, r.out.double()))
    del o64
    ob, _ = _launch(r.what + " (bf16)", size, r.x, r.bank, r.lam, out_dtype=torch.bfloat16)
    want = r.out.to(torch.bfloat16)
    assert torch.equal(ob, want), (r.what, "bf16 output", _first_difference(ob.float(), want.float()))
    del ob
    again, _ = _launch(r.what + " (again)", size, r.x, r.bank, r.lam)
    assert torch.equal(again, r.out), (r.what, "a second call", _first_difference(again, r.out))
    assert _hip.device_status()[0] == 0


@pytest.mark.parametrize("name,gname", lc.WALK_CASES, ids=IDS)
def test_walked_tiles_against_the_exact_model(hip_device, name, gname):
    """c. elementwise at 3 x 2^-23; the worst value measured is in the module's docstring"""
    r = _big(name, gname, str(hip_device))
    CASES_RUN.add(("model", name, gname))
    els = tuple(dict.fromkeys((0, 1, 2, r.B // 2, r.B - 1)))     # first, full, empty, middle, last
    got = lc.checked(name, gname, r.B, els)
    out = r.out[list(els)].cpu().double().numpy()
    model = np.maximum(np.tanh(got.pre.astype(np.float64)), 0.0)
    oracle = np.maximum(np.tanh(got.ref), 0.0)
    err = np.abs(out - model)
    at = tuple(int(i) for i in np.unravel_index(int(err.argmax()), err.shape))
    e_oracle = float(np.abs(out - oracle).max())
    print(f"{r.what} B={r.B} elements {els}: worst |out - model| {err.max():.3e} = {err.max() * 2.0 ** 23:.3f} x 2^-23 "
          f"(bar 3) at element {els[at[0]]} voxel {at[2:]}, pre {got.pre[at]:.6f}; |out - oracle| {e_oracle:.2e}")
    assert not r.out[2].any().item(), (r.what, "the empty element")
    assert err.max() <= A_BAR, (r.what, float(err.max()), els[at[0]], at[2:], float(got.pre[at]), r.plan)
    assert e_oracle < TOL, (r.what, e_oracle)
    assert _hip.device_status()[0] == 0


def test_every_fork_was_walked(hip_device):
    """d. from the plans launched: every fork, store type and the prepared tables, at two or more tiles per workgroup"""
    assert CASES_RUN == {(t, n, g) for t in ("alone", "forms", "model") for n, g in lc.WALK_CASES}, \
        "the coverage check needs the whole module to have run"
    walked = [row for row in RAN if row[1].tiles_per_workgroup_min >= 2]
    seen = {fork: [w for w, p, ks, _, _ in walked if hit(p, ks)] for fork, hit in lc.FORKS.items()}
    for dt in (torch.float32, torch.float64, torch.bfloat16):
        seen[f"{dt} stores"] = [w for w, _, _, d, _ in walked if d == dt]
    seen["prepared tables"] = [w for w, _, _, _, prepared in walked if prepared]
    for fork, whats in seen.items():
        print(f"{fork:32s} {len(whats):3d} launches" + (f", e.g. {whats[0]}" if whats else ": NOT RUN"))
    missing = [fork for fork, whats in seen.items() if not whats]
    assert not missing, f"never run at two or more tiles per workgroup: {missing}"
