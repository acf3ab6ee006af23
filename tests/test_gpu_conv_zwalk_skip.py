"""The z-walk's empty-window skip (csrc/conv_i8z.inc, "EMPTY WINDOWS"; the contraction of SceneNet.forward,
core/models/SCENE_Net.py:322-339): a round whose 9 planes x 9 halo rows hold no set voxel is not run, and nothing about the
results may show it.  The yardstick everywhere is torch.equal ON THE RAW BITS between the default call and the same call
under sn_set_option("conv_i8z_dense", 1), through sn_conv_bank_prepared and _served, on all three conv_i8z_variant shapes;
one case per shape also meets the folded tile kernel (sn_conv_bank without a blob).  The counter (sn_conv_i8z_round_counts)
must say what the numpy restatement of the rule (tools/debug/zwalk_window_rule.py) predicts."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from scene_net_amd import _hip

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("zwalk_window_rule", os.path.join(ROOT, "tools", "debug", "zwalk_window_rule.py"))
rule = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rule)

VARIANTS = (0, 1, 2)
KH = {0: 2, 1: 1, 2: 1}                      # x-rows per round of each variant
SMALL = (1, 1, 12, 8, 64)
ODD = (2, 1, 20, 20, 48)                     # a partial last column in x (20 = 2 x 8 + 4), a partial y tile (48 < 64)
ODD40 = (2, 1, 20, 24, 40)                   # Y % 16 != 0: the walk declines the shape, sn_conv_bank's kernels take the call
CUBE = (1, 1, 64, 64, 64)


def _bank(G, seed, scale=None):
    g = torch.Generator().manual_seed(seed)
    w = torch.rand((G, 9, 9, 9), generator=g) - 0.5
    w = w + w.flip(2)
    w = w + w.flip(3)
    scale = torch.logspace(-2, 0.3, G) if scale is None else scale
    return (w * scale.view(G, 1, 1, 1)).float().contiguous()


def _lam(G, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(G, generator=g) - 0.3) / G


def _bits(t):
    if t is None:
        return None
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def _same(a, b):
    return (a is None and b is None) or torch.equal(_bits(a), _bits(b))


def _call(x, bank, lam, prep, want_act, dt, served):
    c0 = _hip.conv_i8z_round_counts()
    act, out = _hip.conv_bank(x, bank, lam, want_act=want_act, want_out=True, out_dtype=dt, prep=prep, assume_served=served)
    c1 = _hip.conv_i8z_round_counts()
    return act, out, (c1[0] - c0[0], c1[1] - c0[1])


def _twin(x, bank, lam, want_act=False, dt=torch.float32, served=False, prep=None):
    """default call and its dense twin: the same bits; -> (act, out, (run, skipped) of the default call)"""
    prep = _hip.conv_bank_prep(bank) if prep is None else prep
    if served:          # (the caller's word that the verdict is "served": true for these banks; the walk checks it anyway)
        _hip.conv_bank(x, bank, lam, prep=prep)
    act, out, cnt = _call(x, bank, lam, prep, want_act, dt, served)
    with _hip.options(conv_i8z_dense=1):
        act_d, out_d, cnt_d = _call(x, bank, lam, prep, want_act, dt, served)
    assert _same(out, out_d) and _same(act, act_d)
    assert cnt_d[1] == 0 and cnt_d[0] == cnt[0] + cnt[1], (cnt, cnt_d)
    return act, out, cnt


def _everywhere(x, bank, lam, expect=None, groups=1, **kw):
    """on the three variants, through both entries; `expect(kH)` -> the (run, skipped) one launch must report"""
    outs = []
    for v in VARIANTS:
        with _hip.options(conv_i8z_variant=v):
            for served in (False, True):
                act, out, cnt = _twin(x, bank, lam, served=served, **kw)
                if expect is not None:
                    want = expect(KH[v])
                    assert cnt == (groups * want[0], groups * want[1]), (v, served, cnt, want)
                outs.append((act, out))
    for act, out in outs[1:]:
        assert _same(out, outs[0][1]) and _same(act, outs[0][0])
    return outs[0]


def _one_voxel(shape, b, z, xx, y):
    occ = torch.zeros(shape, dtype=torch.bool)
    occ[b, 0, z, xx, y] = True
    return occ


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a HIP device")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def bank16(dev):
    return _bank(16, 3).to(dev), _lam(16, 4).to(dev)


@pytest.mark.parametrize("shape", [SMALL, ODD, CUBE], ids=["12x8x64", "2x20x20x48", "64cubed"])
def test_all_zero_input_skips_every_round(dev, bank16, shape):
    bank, lam = bank16
    x = torch.zeros(shape, dtype=torch.bool, device=dev)
    want_act = shape != CUBE
    act, out = _everywhere(x, bank, lam, expect=lambda kH: rule.counts(np.zeros(shape, bool), kH), want_act=want_act)
    assert rule.counts(np.zeros(shape, bool), 1)[0] == 0
    assert bool((_bits(out) == 0).all())                    # + 0.0 everywhere, - 0.0 nowhere
    if want_act:
        assert bool((_bits(act) == 0).all())
    # the folded tile kernel, once per shape
    a_r, o_r = _hip.conv_bank(x, bank, lam, want_act=want_act, want_out=True)
    assert _same(out, o_r) and _same(act, a_r)


def test_the_shape_the_walk_declines_is_untouched(dev, bank16):
    """2 x 20 x 24 x 40: Y is no multiple of 16, so the prepared entry hands the call to sn_conv_bank's kernels; no round of
    the walk runs or is skipped, and the option changes nothing"""
    bank, lam = bank16
    torch.manual_seed(40)
    x = (torch.rand(ODD40) < 0.02).to(dev)
    _everywhere(x, bank, lam, expect=lambda kH: (0, 0))


def _voxel_cases(shape):
    _, _, Z, X, Y = shape
    zs, xs, ys = sorted({0, Z // 2, Z - 1}), sorted({0, X // 2, X - 1}), sorted({0, Y // 2, Y - 1})
    return [(z, xx, y) for z in zs for xx in xs for y in ys]


def test_one_voxel_interior_runs_81_rounds(dev, bank16):
    bank, lam = bank16
    shape = (1, 1, 20, 24, 64)                               # single y tile; the voxel's window lies inside the grid
    occ = _one_voxel(shape, 0, 10, 11, 30)
    assert rule.counts(occ.numpy(), 1)[0] == 81
    _, out = _everywhere(occ.to(dev), bank, lam, expect=lambda kH: rule.counts(occ.numpy(), kH))
    assert _same(out, _hip.conv_bank(occ.to(dev), bank, lam)[1])


@pytest.mark.parametrize("shape", [SMALL, ODD], ids=["12x8x64", "2x20x20x48"])
def test_one_voxel_at_every_face_edge_and_corner(dev, bank16, shape):
    bank, lam = bank16
    for z, xx, y in _voxel_cases(shape):
        occ = _one_voxel(shape, shape[0] - 1, z, xx, y)
        for v in VARIANTS:
            with _hip.options(conv_i8z_variant=v):
                _, _, cnt = _twin(occ.to(dev), bank, lam)
            lo, hi = rule.counts_exact(occ.numpy(), KH[v]), rule.counts(occ.numpy(), KH[v])
            assert lo[0] <= cnt[0] <= hi[0] and cnt == hi, (z, xx, y, v, cnt, lo, hi)


@pytest.mark.parametrize("axis", ["z", "x"])
@pytest.mark.parametrize("dist", [4, 5])
def test_a_voxel_at_distance_4_and_5_from_a_probed_row(dev, bank16, axis, dist):
    """the probed output row (z, x) = (10, 12) is in the voxel's window at distance 4 and outside it at 5"""
    bank, lam = bank16
    shape = (1, 1, 24, 24, 64)
    for sign in (-1, 1):
        z, xx = (10 + sign * dist, 12) if axis == "z" else (10, 12 + sign * dist)
        occ = _one_voxel(shape, 0, z, xx, 17)
        _, out = _everywhere(occ.to(dev), bank, lam, expect=lambda kH: rule.counts(occ.numpy(), kH))
        a_r, o_r = _hip.conv_bank(occ.to(dev), bank, lam, want_act=True, want_out=True)
        assert _same(out, o_r)
        assert bool((a_r[0, :, 10, 12] != 0).any()) == (dist == 4)


@pytest.mark.parametrize("xx,which", [(0, "first"), (13, "second")])
def test_a_voxel_that_makes_only_one_round_of_a_ticket_non_empty(dev, bank16, xx, which):
    """variant 2's tickets hold the x-rows (2 k, 2 k + 1) of a column.  A voxel at x = 0 reaches rows 0 .. 4: of the ticket
    (4, 5) only its first round; a voxel at x = 13 reaches rows 9 .. 17: of the ticket (8, 9) only its second."""
    bank, lam = bank16
    shape = (1, 1, 12, 24, 64)
    occ = _one_voxel(shape, 0, 6, xx, 40)
    _, out = _everywhere(occ.to(dev), bank, lam, expect=lambda kH: rule.counts(occ.numpy(), kH))
    a_r, o_r = _hip.conv_bank(occ.to(dev), bank, lam, want_act=True, want_out=True)
    assert _same(out, o_r)
    lone, empty = (4, 5) if which == "first" else (9, 8)
    assert bool((a_r[0, :, 6, lone] != 0).any()) and not bool((a_r[0, :, 6, empty] != 0).any())


@pytest.mark.parametrize("shape", [SMALL, ODD], ids=["12x8x64", "2x20x20x48"])
def test_half_occupancy_skips_nothing(dev, bank16, shape):
    bank, lam = bank16
    torch.manual_seed(50)
    occ = torch.rand(shape) < 0.5
    assert rule.counts(occ.numpy(), 1)[1] == 0
    act, out = _everywhere(occ.to(dev), bank, lam, expect=lambda kH: rule.counts(occ.numpy(), kH), want_act=True)
    a_r, o_r = _hip.conv_bank(occ.to(dev), bank, lam, want_act=True, want_out=True)
    assert _same(out, o_r) and _same(act, a_r)


def test_a_synthetic_tile_at_64_cubed(dev, bank16):
    import scene_net_amd as sna
    from scene_net_amd.synthetic import synthetic_tile
    bank, lam = bank16
    tile = synthetic_tile(3, 100_000)[0]
    occ = sna.voxelize_batch(sna.PointBatch.from_tiles([tile], device=dev), (64,) * 3, occ_dtype=torch.bool).occ
    host = occ.cpu().numpy()
    assert rule.counts(host, 1)[1] > 0 and rule.counts(host, 1)[0] > 0
    _, out = _everywhere(occ, bank, lam, expect=lambda kH: rule.counts(host, kH))
    assert _same(out, _hip.conv_bank(occ, bank, lam)[1])


@pytest.mark.parametrize("dt", [torch.float32, torch.float64], ids=["fp32", "fp64"])
def test_activations_wanted(dev, bank16, dt):
    bank, lam = bank16
    torch.manual_seed(60)
    occ = torch.zeros(ODD, dtype=torch.bool)
    occ[:, :, 2:9, 3:7] = torch.rand((2, 1, 7, 4, 48)) < 0.3        # a busy corner, the rest empty
    act, out = _everywhere(occ.to(dev), bank, lam, expect=lambda kH: rule.counts(occ.numpy(), kH), want_act=True, dt=dt)
    assert rule.counts(occ.numpy(), 1)[1] > 0
    a_r, o_r = _hip.conv_bank(occ.to(dev), bank, lam, want_act=True, want_out=True, out_dtype=dt)
    assert _same(out, o_r) and _same(act, a_r)
    assert act.dtype == dt and out.dtype == dt


def test_twenty_kernels_accumulate_over_skipped_rounds(dev):
    """G = 20: two groups; the second launch adds to what the first stored (head & 1), then applies the head.  Under a skipped
    round the first pass stored + 0.0; the load-and-add and relu_tanh still run, from e = + 0.0.  (The first pass's values
    come from the launch itself: the entry takes no pre-filled `out`, so - 0.0 cannot be planted there from outside.)"""
    bank, lam = _bank(20, 7).to(dev), _lam(20, 8).to(dev)
    torch.manual_seed(70)
    occ = torch.zeros(ODD, dtype=torch.bool)
    occ[:, :, 12:, 10:] = torch.rand((2, 1, 8, 10, 48)) < 0.2
    for dt in (torch.float32, torch.float64):
        act, out = _everywhere(occ.to(dev), bank, lam, expect=lambda kH: rule.counts(occ.numpy(), kH), groups=2,
                               want_act=True, dt=dt)
        a_r, o_r = _hip.conv_bank(occ.to(dev), bank, lam, want_act=True, want_out=True, out_dtype=dt)
        assert _same(out, o_r) and _same(act, a_r)


@pytest.mark.parametrize("shape", [(1, 1, 64, 8, 64), (1, 1, 40, 16, 64)], ids=["64x8x64", "40x16x64"])
def test_few_columns_several_jobs_per_stream(dev, bank16, shape):
    """one or two columns: the host cuts them into z segments (a last one shorter than the others at Z = 40)"""
    bank, lam = bank16
    torch.manual_seed(80)
    occ = torch.zeros(shape, dtype=torch.bool)
    occ[0, 0, 5, 3, 20] = True
    occ[0, 0, shape[2] - 2, shape[3] - 1, 63] = True
    occ[0, 0, shape[2] // 2, :, :] = torch.rand(shape[3:]) < 0.1
    act, out = _everywhere(occ.to(dev), bank, lam, expect=lambda kH: rule.counts(occ.numpy(), kH), want_act=True)
    assert rule.counts(occ.numpy(), 1)[1] > 0
    a_r, o_r = _hip.conv_bank(occ.to(dev), bank, lam, want_act=True, want_out=True)
    assert _same(out, o_r) and _same(act, a_r)


@pytest.mark.parametrize("bad,guard", [(float("inf"), 1), (float("inf"), 0), (float("nan"), 1), (float("nan"), 0)],
                         ids=["inf", "inf_guard_off", "nan", "nan_guard_off"])
def test_a_non_finite_coefficient_switches_the_skip_off(dev, bank16, bad, guard):
    """NaN passes the quantisation guard (no comparison with NaN holds) and reaches the walk; inf makes the guard's bound
    infinite, so the walk hands the launch to the fp32 form unless the guard is off (conv_i8_tolerance_ppb = 0).  Wherever
    the walk serves such a bank it runs every round: inf x 0 and NaN x 0 are NaN, as in dense mode."""
    bank, lam = bank16
    lam = lam.clone()
    lam[5] = bad
    occ = _one_voxel(SMALL, 0, 6, 4, 30)
    assert rule.counts(occ.numpy(), 1)[1] > 0          # (rounds the skip would take, were it on)
    walk_serves = not (bad == float("inf") and guard)
    tol = {} if guard else {"conv_i8_tolerance_ppb": 0}
    with _hip.options(**tol):
        for v in VARIANTS:
            with _hip.options(conv_i8z_variant=v):
                for served in ((False, True) if walk_serves else (False,)):
                    _, out, cnt = _twin(occ.to(dev), bank, lam, served=served)
                    assert cnt == ((sum(rule.counts(occ.numpy(), KH[v])), 0) if walk_serves else (0, 0)), cnt
        ref = _hip.conv_bank(occ.to(dev), bank, lam)[1]
    assert bool(torch.isnan(out).any())
    if walk_serves:
        assert torch.equal(torch.isnan(out), torch.isnan(ref))
    assert _hip.device_status()[0] == 0


def test_a_bank_the_walk_declines(dev, bank16):
    _, lam = bank16
    asym = _bank(16, 4)
    asym[3, 2, 1, 7] += 0.125
    wide = _bank(16, 3, scale=torch.full((16,), 40.0))     # over the quantisation tolerance
    occ = _one_voxel(SMALL, 0, 6, 4, 30).to(dev)
    for bank in (asym.to(dev), wide.to(dev)):
        prep = _hip.conv_bank_prep(bank)
        for v in VARIANTS:
            with _hip.options(conv_i8z_variant=v):
                p0 = _hip.conv_i8_path_counts()
                act, out, cnt = _call(occ, bank, lam, prep, True, torch.float32, False)
                p1 = _hip.conv_i8_path_counts()
                with _hip.options(conv_i8z_dense=1):
                    act_d, out_d, cnt_d = _call(occ, bank, lam, prep, True, torch.float32, False)
                p2 = _hip.conv_i8_path_counts()
            assert _same(out, out_d) and _same(act, act_d)
            assert tuple(b - a for a, b in zip(p0, p1)) == tuple(b - a for a, b in zip(p1, p2))
            assert cnt == (0, 0) and cnt_d == (0, 0)          # not served by the walk: no round at all
        a_r, o_r = _hip.conv_bank(occ, bank, lam, want_act=True, want_out=True)
        assert _same(out, o_r) and _same(act, a_r)
    assert _hip.device_status()[0] == 0


def _three_calls(x, fills, bank, lam, prep, act, out, results):
    """50 % input, all-zero input, the 50 % input again -- through the SAME input and output buffers"""
    fn = _hip.load().sn_conv_bank_prepared
    B, _, Z, X, Y = x.shape
    for i, f in enumerate(fills):
        x.copy_(f)
        rc = fn(x.data_ptr(), _hip.SN_OCC8, bank.data_ptr(), lam.data_ptr(), prep.data_ptr(), B, Z, X, Y, 16, 9, 9, 9,
                act.data_ptr(), out.data_ptr(), _hip.SN_F32, torch.cuda.current_stream().cuda_stream)
        assert rc == 0
        results[i][0].copy_(act)
        results[i][1].copy_(out)


def test_same_buffers_three_calls_eager_and_captured(dev, bank16):
    """no mask outlives its plane: the all-zero call between two busy ones, eagerly and as one captured graph replayed after
    the inputs were refilled; every result equals its dense twin"""
    bank, lam = bank16
    prep = _hip.conv_bank_prep(bank)
    torch.manual_seed(90)
    shape = ODD
    half, half2 = (torch.rand(shape) < 0.5).to(dev), (torch.rand(shape) < 0.5).to(dev)
    zero = torch.zeros(shape, dtype=torch.bool, device=dev)
    fills = [half.clone(), zero.clone(), half.clone()]       # (static tensors: a replay copies from them)
    x = torch.empty(shape, dtype=torch.bool, device=dev)
    act = torch.empty((shape[0], 16) + shape[2:], device=dev)
    out = torch.empty(shape, device=dev)
    new = lambda: [(torch.empty_like(act), torch.empty_like(out)) for _ in range(3)]
    for v in VARIANTS:
        with _hip.options(conv_i8z_variant=v):
            eager, eager_d = new(), new()
            _three_calls(x, fills, bank, lam, prep, act, out, eager)
            with _hip.options(conv_i8z_dense=1):
                _three_calls(x, fills, bank, lam, prep, act, out, eager_d)
            torch.cuda.synchronize()
            for (a, o), (a_d, o_d) in zip(eager, eager_d):
                assert _same(a, a_d) and _same(o, o_d)
            assert _same(eager[0][1], eager[2][1]) and bool((_bits(eager[1][1]) == 0).all())
            # one graph per mode (the option is read when the launch is enqueued, i.e. captured)
            got, got_d = new(), new()
            graphs = []
            for dense, res in ((0, got), (1, got_d)):
                with _hip.options(conv_i8z_dense=dense):
                    g = torch.cuda.CUDAGraph()
                    side = torch.cuda.Stream()
                    side.wait_stream(torch.cuda.current_stream())
                    with torch.cuda.stream(side):
                        with torch.cuda.graph(g, stream=side):
                            _three_calls(x, fills, bank, lam, prep, act, out, res)
                    torch.cuda.current_stream().wait_stream(side)
                    graphs.append(g)
            fills[0].copy_(half2)
            fills[2].copy_(half2)
            for g in graphs:
                g.replay()
            torch.cuda.synchronize()
            for (a, o), (a_d, o_d) in zip(got, got_d):
                assert _same(a, a_d) and _same(o, o_d)
            ref = _hip.conv_bank(half2, bank, lam, want_act=True, want_out=True)
            assert _same(got[0][0], ref[0]) and _same(got[2][1], ref[1]) and bool((_bits(got[1][1]) == 0).all())
            fills[0].copy_(half)
            fills[2].copy_(half)
    assert _hip.device_status()[0] == 0


def test_injected_fault_on_an_all_zero_input_is_still_loud(dev, bank16):
    """a skipped round bypasses no check: the dependency that never arrives (the existing test hook, once) still ends in NaN
    outputs, the latched sticky status and a counted give-up"""
    bank, lam = bank16
    x = torch.zeros((2, 1, 16, 24, 64), dtype=torch.bool, device=dev)
    prep = _hip.conv_bank_prep(bank)
    good_a, good_o = _hip.conv_bank(x, bank, lam, want_act=True, want_out=True, prep=prep)
    t0 = _hip.conv_i8_spin_timeouts()
    assert _hip.device_status()[0] == 0
    try:
        with _hip.options(conv_i8z_inject_fault=1):
            act, out = _hip.conv_bank(x, bank, lam, want_act=True, want_out=True, prep=prep)
        torch.cuda.synchronize()
        assert bool(torch.isnan(out).all()) and bool(torch.isnan(act).all())
        assert _hip.device_status()[0] == 1
        with pytest.raises(_hip.HipLibraryError, match="latched status"):
            _hip.conv_bank_prep(torch.zeros((16, 9, 9, 9), device=dev))
    finally:
        _hip.device_status_clear()
    assert _hip.device_status()[0] == 0 and _hip.conv_i8_spin_timeouts() > t0
    act2, out2 = _hip.conv_bank(x, bank, lam, want_act=True, want_out=True, prep=prep)
    torch.cuda.synchronize()
    assert _same(act2, good_a) and _same(out2, good_o) and bool((_bits(out2) == 0).all())
