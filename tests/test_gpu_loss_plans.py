"""K5 (scene-net_amd/csrc/loss.hip) at every launch plan it can pick: part counts and spans of both passes (one part, exact
and uneven splits, the 256 / 512 caps), vector and element loop, the three target paths with ties, extremes and every byte
class, every term mask, batches on either side of the combine kernel's 1024 threads, and the penalties at every size up to
the documented 8192.  The plan itself is restated in tests/loss_cases.py and pinned on the CPU in tests/test_host_logic.py.

What a stale buffer could hide is made visible: every gradient is written into a buffer filled with NaN beforehand
(`_hip.loss_backward(out=)`), and `_forward` hands sn_loss_forward_m statistics / loss / coefficient buffers filled with NaN
too -- the caching allocator otherwise returns the block of the previous call, which holds a correct result."""
import numpy as np
import pytest
import torch

import scene_net_amd as sna
from scene_net_amd import _hip
from oracle import loss_oracle as lo
import loss_cases as lc

pytestmark = pytest.mark.gpu

NAN = float("nan")
K = _hip.SN_LOSS_MAX_BINS
WMSE, FOCAL, DICE, WBCE = _hip.SN_LOSS_WMSE, _hip.SN_LOSS_FOCAL_TVERSKY, _hip.SN_LOSS_DICE, _hip.SN_LOSS_WBCE
RANGES10 = torch.linspace(0, 1, 11)[:-1]
RANGES16 = torch.linspace(0, 1, 17)[:-1]
FREQS16 = lc.FREQS + [500, 20000, 70, 2500, 1100, 60]
CFG = dict(mse_weight=lc.HP["mse_weight"], dice_smooth=1.0, **lc.TVERSKY)


def _forward(pred, gt, ranges, bin_w, terms, **cfg):
    """_hip.loss_forward with buffers of the test's own, filled with NaN: (loss [5], stats [B, 3H+5], coef, loss32 [5]).
    Nothing the two launches should have written may still be NaN."""
    B, H = int(pred.shape[0]), int(ranges.numel())
    n_per = pred.numel() // B
    dev = pred.device
    ws = torch.full((B * _hip.loss_parts(n_per) * (3 * H + 5),), NAN, dtype=torch.float64, device=dev)
    stats = torch.full((B, 3 * H + 5), NAN, dtype=torch.float64, device=dev)
    loss = torch.full((5,), NAN, dtype=torch.float64, device=dev)
    loss32 = torch.full((5,), NAN, dtype=torch.float32, device=dev)
    coef = torch.full((2 * K + 3 * B,), NAN, dtype=torch.float64, device=dev)
    c = dict(mse_weight=1.0, tversky_alpha=0.5, tversky_beta=1.0, focal_gamma=1.0, tversky_smooth=1.0, dice_smooth=1.0)
    c.update(cfg)
    assert pred.is_contiguous() and gt.is_contiguous() and ranges.dtype == bin_w.dtype == torch.float32
    with torch.cuda.device(dev):
        rc = _hip.load().sn_loss_forward_m(pred.data_ptr(), _hip._DT[pred.dtype], gt.data_ptr(), _hip._DT[gt.dtype], B, n_per,
                                           ranges.data_ptr(), bin_w.data_ptr(), H, int(terms), c["mse_weight"],
                                           c["tversky_alpha"], c["tversky_beta"], c["focal_gamma"], c["tversky_smooth"],
                                           c["dice_smooth"], ws.data_ptr(), stats.data_ptr(), loss.data_ptr(),
                                           loss32.data_ptr(), coef.data_ptr(), _hip._stream())
    assert rc == 0, _hip.load().sn_last_error()
    for name, t in (("parts", ws), ("stats", stats), ("loss", loss), ("loss32", loss32), ("coef", coef)):
        assert not torch.isnan(t).any().item(), f"sn_loss_forward_m left {name} unwritten"
    return loss, stats, coef, loss32


def _grad(pred, gt, ranges, coef, upstream=None):
    """_hip.loss_backward into a buffer filled with NaN: an element that no part wrote stays NaN."""
    out = torch.full_like(pred, NAN)
    got = _hip.loss_backward(pred, gt, ranges, coef, upstream, out=out)
    assert got is out
    assert not torch.isnan(out).any().item(), "sn_loss_backward left gradient elements unwritten"
    return out


def _poison(like):
    """Frees a block of like's size filled with NaN: the caching allocator's candidate for the next empty_like(like), so a
    wrapper that allocates its own output is less likely to be handed an earlier, correct result."""
    torch.full_like(like, NAN)


def _check_integer_stats(stats, gt, ranges):
    """Exact: stats[b, :H] is the oracle's count per nearest bin; for byte targets stats[b, 2H+2] is the sum of the targets
    (the number of ones of a binary one)."""
    B, H = gt.shape[0], ranges.numel()
    flat = lc.as_oracle_target(gt).reshape(B, -1)
    idx = lo.nearest_bin(flat, ranges)
    want = torch.zeros((B, H), dtype=torch.int64).scatter_add_(1, idx, torch.ones_like(idx))
    assert torch.equal(want[0], torch.bincount(idx[0], minlength=H))
    got = stats.cpu()
    assert torch.equal(got[:, :H], want.double()), (got[:, :H] - want.double()).abs().max().item()
    if gt.dtype in (torch.bool, torch.uint8):
        assert torch.equal(got[:, 2 * H + 2], gt.reshape(B, -1).long().sum(dim=1).double())


def _compare(tag, loss, grad, ref, gref, tol):
    """|loss - ref| <= tol |ref| and max|grad - gref| <= tol max|gref|; the figures are printed before they are judged."""
    e_loss = abs(loss - ref) / abs(ref)
    e_grad = (grad.cpu().double() - gref).abs().max().item() / gref.abs().max().item()
    print(f"{tag}: loss error {e_loss:.3g}, gradient error {e_grad:.3g}, tolerance {tol:g}")
    assert e_loss <= tol, (tag, loss, ref)
    assert e_grad <= tol, (tag, e_grad)


def _tversky_case(dev, pred, gt, ranges=None, freqs=lc.FREQS):
    """The case of test_against_oracle_all_dtypes_and_ragged_shapes (weighted MSE + focal Tversky through
    sna.GENEO_Tversky_Loss) with its statistics and a gradient written over NaN: (loss, stats, grad)."""
    crit = lc.tversky_criterion(dev, freqs, ranges)
    r, bin_w = crit._device_tables(dev)
    terms, cfg = crit._terms()
    pd, gd = pred.to(dev), gt.to(dev)
    loss, stats, coef, loss32 = _forward(pd, gd, r, bin_w, terms, mse_weight=crit.mse_weight, **cfg)
    via_class = crit(pd, gd, {}, {})   # the criterion returns the same number, rounded once to pred's precision
    assert via_class.item() == (loss[0] if pred.dtype == torch.float64 else loss32[0]).item()
    return loss[0].item(), stats, _grad(pd, gd, r, coef)


# ------------------------------------------------------------------ 1. every plan against the fp64 oracle
def _plan_case(dev, shape, pred_dt, gt_dt):
    pred, gt = lc.seeded_inputs(shape, pred_dt, gt_dt)
    ref, gref = lc.tversky_oracle(pred, gt)
    loss, stats, grad = _tversky_case(dev, pred, gt)
    _check_integer_stats(stats, gt, RANGES10)
    _compare(f"plan {lc.plan(shape[1])} {pred_dt} {gt_dt}", loss, grad, ref, gref, lc.oracle_tol(pred_dt))


@pytest.mark.parametrize("pred_dt,gt_dt", lc.DTYPE_PAIRS)
@pytest.mark.parametrize("n_per", lc.SMALL_N)
def test_small_plans_against_oracle(hip_device, n_per, pred_dt, gt_dt):
    """One part, exact and uneven splits below the caps, vector and element loop (tests/loss_cases.py), B = 3, all six
    dtype pairs: loss and gradient against the fp64 oracle at 5e-6 (fp32 predictions) / 1e-6 (fp64), counts exact.
    Measured on an MI355X over the 48 cases: loss error at most 1.4e-7, gradient error at most 2.9e-7 (fp32 predictions)
    and 1.3e-7 (fp64)."""
    _plan_case(hip_device, (3, n_per), pred_dt, gt_dt)


@pytest.mark.parametrize("pred_dt,gt_dt", [(torch.float32, torch.bool), (torch.float32, torch.float32),
                                           (torch.float64, torch.float64)])
@pytest.mark.parametrize("n_per", lc.LARGE_N)
def test_capped_plans_against_oracle(hip_device, n_per, pred_dt, gt_dt):
    """256 forward and 512 backward parts: exact split, element loop, uneven split, spans beyond 16384 / 8192; B = 1.
    Measured on an MI355X over the 12 cases: loss error at most 9.9e-8, gradient error at most 3.4e-7 (fp32 predictions,
    tolerance 5e-6) and 1.9e-7 (fp64, tolerance 1e-6)."""
    _plan_case(hip_device, (1, n_per), pred_dt, gt_dt)


# ------------------------------------------------------------------ 2. exact probes at the part boundaries
def _probe_positions(n_per, which):
    """First, second, last-but-one and last part of one pass's plan: lo, lo+1, lo+3, hi-4, hi-1; element 0 and n_per-1."""
    fp, fs, bp, bs, _ = lc.plan(n_per)
    bounds = lc.part_bounds(n_per, *((fp, fs) if which == "forward" else (bp, bs)))
    pos = {0, n_per - 1}
    for a, b in {bounds[0], bounds[min(1, len(bounds) - 1)], bounds[max(len(bounds) - 2, 0)], bounds[-1]}:
        assert b - a >= 8
        pos.update((a, a + 1, a + 3, b - 4, b - 1))
    assert len(pos) <= 24   # 4^-24 = 2^-48: every partial sum of the squares fits fp64's 53 bits
    return sorted(pos)


@pytest.mark.parametrize("which", ["forward", "backward"])
@pytest.mark.parametrize("gt_dt", [torch.bool, torch.float32])
@pytest.mark.parametrize("pred_dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("n_per", [16388, 16385, 8196, 4_194_308, 4_194_307])
def test_probes_at_part_boundaries_sum_exactly(hip_device, n_per, pred_dt, gt_dt, which):
    """pred is 0 except 2^-(j+1) at the j-th probe, gt is 0: every sum below is exact in fp64 whatever its order, so an
    element dropped or taken twice at a part's edge changes a bit of it.  With the weighted MSE alone the gradient is one
    fp32 product per element, c[bin of 0] * pred, exact as well (a power of two times the coefficient)."""
    pos = _probe_positions(n_per, which)
    vals = 2.0 ** -(torch.arange(len(pos), dtype=torch.float64) + 1)
    pred = torch.zeros((1, n_per), dtype=pred_dt)
    pred[0, pos] = vals.to(pred_dt)
    assert torch.equal(pred[0, pos].double(), vals)
    pred = pred.to(hip_device)
    gt = torch.zeros((1, n_per), dtype=gt_dt, device=hip_device)
    ranges, bin_w = RANGES10.to(hip_device), torch.linspace(0.1, 1.0, 10).to(hip_device)
    _, stats, coef, _ = _forward(pred, gt, ranges, bin_w, WMSE)
    s, H = stats[0].cpu(), 10
    assert s[2 * H + 1].item() == vals.sum().item()            # sum of pred
    assert s[2 * H + 3].item() == (vals * vals).sum().item()   # sum of pred^2
    assert s[H + 0].item() == (vals * vals).sum().item()       # squared error of the bin of target 0
    assert s[:H].sum().item() == n_per and s[0].item() == n_per
    assert s[2 * H].item() == 0 and s[2 * H + 2].item() == 0 and s[2 * H + 4].item() == 0
    grad = _grad(pred, gt, ranges, coef)
    assert torch.equal(grad, (coef[0].float() * pred.float()).to(pred_dt))


# ------------------------------------------------------------------ 3. bins: ties, extremes, byte values
def _tie_targets(ranges, dt):
    """Every range value, every midpoint of two neighbours formed in the target's dtype, its two neighbours in that
    dtype, and 1.0."""
    r = ranges.to(dt)
    mid = (r[:-1] + r[1:]) / 2
    return torch.cat([r, mid, torch.nextafter(mid, torch.full_like(mid, 2.0)),
                      torch.nextafter(mid, torch.full_like(mid, -1.0)), torch.ones(1, dtype=dt)])


@pytest.mark.parametrize("gt_dt", [torch.float32, torch.float64, torch.uint8])
@pytest.mark.parametrize("shape", [(2, 16385), (2, 16388)])
@pytest.mark.parametrize("H", [1, 10, 16])
def test_bins_ties_extremes_and_byte_values(hip_device, H, shape, gt_dt):
    """Float targets on the bin centres, on the exact ties between two of them (first minimum wins, w_mse.py:122) and one
    ulp to either side; byte targets over the whole table, not only 0 and 1.  Counts exact, loss and gradient at the
    tolerances of the plan tests (measured on an MI355X: loss error at most 2.4e-7, gradient error at most 2.7e-7 for fp32
    and 1.7e-7 for fp64 predictions)."""
    ranges = {1: torch.zeros(1), 10: RANGES10, 16: RANGES16}[H]
    freqs = FREQS16 if H == 16 else lc.FREQS
    if gt_dt == torch.uint8:
        vals = torch.tensor([0, 1, 2, 7, 128, 255], dtype=torch.uint8)
    else:
        vals = _tie_targets(ranges, gt_dt)
        if H > 1:   # the set does hold true ties in the arithmetic of the search
            d = (vals.unsqueeze(-1) - ranges).abs().sort(dim=-1).values
            assert (d[:, 0] == d[:, 1]).sum().item() >= 1
    n = shape[0] * shape[1]
    gt = vals[torch.arange(n) % len(vals)].reshape(shape)
    pred_dt = torch.float64 if gt_dt == torch.float64 else torch.float32
    pred = torch.rand(shape, generator=torch.Generator().manual_seed(H + shape[1]), dtype=torch.float64).to(pred_dt)
    ref, gref = lc.tversky_oracle(pred, gt, freqs, ranges)
    loss, stats, grad = _tversky_case(hip_device, pred, gt, ranges, freqs)
    _check_integer_stats(stats, gt, ranges)
    _compare(f"bins H={H} {shape} {gt_dt}", loss, grad, ref, gref, lc.oracle_tol(pred_dt))


# ------------------------------------------------------------------ 4. every term mask
def _mask_tol(dtype):
    """_tol of tests/test_gpu_loss.py: the BCE logarithm and the gradient arithmetic are taken in pred's dtype."""
    return 2e-5 if dtype == torch.float32 else 1e-6


@pytest.mark.parametrize("binary", [False, True])
@pytest.mark.parametrize("pred_dt", [torch.float32, torch.float64])
@pytest.mark.parametrize("shape", [(3, 16385), (3, 8196)])
def test_every_term_mask(hip_device, shape, pred_dt, binary):
    """All 15 non-empty masks of WMSE | FOCAL_TVERSKY | DICE | WBCE: each requested term equals its own oracle, the others
    are exactly 0, loss[0] is their sum, the gradient is autograd's of the same sum; an upstream scalar of 4 (a power of
    two: every product scales exactly) multiplies the gradient bit for bit, read as fp64 or as fp32.  Measured on an
    MI355X: term error at most 2.9e-7, gradient error at most 3.4e-7, in either dtype (tolerances 2e-5 / 1e-6)."""
    pred, gt = lc.seeded_inputs(shape, pred_dt, torch.bool if binary else pred_dt)
    pred = pred.clamp(1e-4, 1 - 1e-4)
    freqs, a, e = torch.tensor(lc.FREQS), lc.HP["alpha"], lc.HP["eps"]
    po = pred.double().requires_grad_(True)
    gto = lc.as_oracle_target(gt)
    tv = lc.TVERSKY
    w = lo.weight_target(gto, freqs, RANGES10, a, e).double()
    ref_terms = {
        WMSE: lo.weighted_mse(po, gto, freqs, RANGES10, a, e, lc.HP["mse_weight"]),
        FOCAL: lo.focal_tversky_loss(po, gto.double(), tv["tversky_alpha"], tv["tversky_beta"], tv["focal_gamma"],
                                     tv["tversky_smooth"]),
        DICE: lo.binary_dice_loss(po, gto.double()),
        WBCE: torch.mean(w * torch.nn.functional.binary_cross_entropy(po, gto.double(), reduction="none")),
    }
    ranges = RANGES10.to(hip_device)
    bin_w = lo.bin_weights(freqs, a, e, 10).float().to(hip_device)
    pd, gd = pred.to(hip_device), gt.to(hip_device)
    up64 = torch.tensor([4.0], dtype=torch.float64, device=hip_device)
    tol = _mask_tol(pred_dt)
    worst = [0.0, 0.0]
    for mask in range(1, 16):
        ref = sum(t for bit, t in ref_terms.items() if mask & bit)
        gref, = torch.autograd.grad(ref, po, retain_graph=True)
        loss, _, coef, loss32 = _hip.loss_forward(pd, gd, ranges, bin_w, mask, **CFG)
        l = loss.cpu()
        for slot, bit in enumerate((WMSE, FOCAL, DICE, WBCE), start=1):
            if mask & bit:
                want = ref_terms[bit].item()
                worst[0] = max(worst[0], abs(l[slot].item() - want) / abs(want))
                assert abs(l[slot].item() - want) <= tol * abs(want), (mask, slot, l[slot].item(), want)
            else:
                assert l[slot].item() == 0.0, (mask, slot)
        assert abs(l[0].item() - (l[1] + l[2] + l[3] + l[4]).item()) < 1e-12
        assert torch.equal(loss32.cpu(), l.float())
        g1 = _grad(pd, gd, ranges, coef)
        err = (g1.cpu().double() - gref).abs().max().item() / gref.abs().max().item()
        worst[1] = max(worst[1], err)
        assert err <= tol, (mask, err)
        g4 = _grad(pd, gd, ranges, coef, up64)
        assert torch.equal(g4, 4 * g1), mask
        assert torch.equal(_grad(pd, gd, ranges, coef, up64.float()), g4), mask
    print(f"masks {shape} {pred_dt} binary={binary}: term error {worst[0]:.3g}, gradient error {worst[1]:.3g}, "
          f"tolerance {tol:g}")


# ------------------------------------------------------------------ 5. batch sizes
@pytest.mark.parametrize("n_per", [36, 37])
@pytest.mark.parametrize("B", [1, 7, 8, 9, 1023, 1024, 1025, 2500])
def test_batch_sizes_around_the_combine_block(hip_device, B, n_per):
    """loss_combine_kernel walks samples in blocks of 8 then 1 and stripes the per-sample dice term and gradient
    coefficients over 1024 threads: from sample 1024 on they come from a second trip.  WMSE | FOCAL_TVERSKY | DICE against
    the oracle (binary_dice_loss, reduction mean), fp32 and fp64 predictions, binary and float targets.  Measured on an
    MI355X: loss error at most 7.4e-8, gradient error at most 2.9e-7 (fp32) and 2.0e-7 (fp64)."""
    ranges = RANGES10.to(hip_device)
    freqs = torch.tensor(lc.FREQS)
    bin_w = lo.bin_weights(freqs, lc.HP["alpha"], lc.HP["eps"], 10).float().to(hip_device)
    for pred_dt in (torch.float32, torch.float64):
        for gt_dt in (torch.bool, pred_dt):
            pred, gt = lc.seeded_inputs((B, n_per), pred_dt, gt_dt)
            po = pred.double().requires_grad_(True)
            gto = lc.as_oracle_target(gt)
            tv = lc.TVERSKY
            ref = lo.weighted_mse(po, gto, freqs, RANGES10, lc.HP["alpha"], lc.HP["eps"], lc.HP["mse_weight"]) + \
                lo.focal_tversky_loss(po, gto.double(), tv["tversky_alpha"], tv["tversky_beta"], tv["focal_gamma"],
                                      tv["tversky_smooth"]) + lo.binary_dice_loss(po, gto.double())
            ref.backward()
            pd, gd = pred.to(hip_device), gt.to(hip_device)
            loss, stats, coef, _ = _forward(pd, gd, ranges, bin_w, WMSE | FOCAL | DICE, **CFG)
            _check_integer_stats(stats, gt, RANGES10)
            _compare(f"batch {B} x {n_per} {pred_dt} {gt_dt}", loss[0].item(), _grad(pd, gd, ranges, coef), ref.item(),
                     po.grad, lc.oracle_tol(pred_dt))


# ------------------------------------------------------------------ 6. penalties at every size
PEN_W = 1.5


def _penalty_inputs(N, over):
    """P uniform in [-1, 1]; mask of 0 / 1 / 2 in mixed order with one of each where N allows; the mask == 2 entries
    scaled so that their sum is 1.5 (over: the frozen coefficient 1 - sum is negative) or 0.5."""
    rng = np.random.default_rng(1000 + N)
    P = rng.uniform(-1.0, 1.0, N)
    mask = rng.integers(0, 3, N).astype(np.int8)
    mask[:3] = np.array([2, 1, 0], dtype=np.int8)[:N]
    free = mask == 2
    P[free] *= (1.5 if over else 0.5) / P[free].sum()
    P = P.astype(np.float32)
    # the sign decision stays clear of fp32 rounding: |1 - sum| >= 0.1, the kernel's summation error below a tenth of that
    assert abs(1.0 - P[free].astype(np.float64).sum()) >= 0.1
    assert (N / 256 + 16) * 2.0 ** -24 * (1.0 + np.abs(P[free]).sum()) < 0.01
    return P, mask


def _penalty_oracle(P, mask, with_sum):
    """fp64: (value, sum of the magnitudes that entered it, gradient [N] as the kernel's fp32 w * {0, -1, +1})."""
    v = P.astype(np.float64)
    relu = np.maximum(-v, 0.0)[mask >= 1].sum()
    last = 1.0 - v[mask == 2].sum()
    last_neg = bool(with_sum) and last < 0
    value = PEN_W * (relu + (-last if last_neg else 0.0))
    mag = relu + ((1.0 + np.abs(v[mask == 2]).sum()) if last_neg else 0.0)
    g = -1.0 * ((mask >= 1) & (v < 0)) + 1.0 * ((mask == 2) & last_neg)
    return value, mag, (np.float32(PEN_W) * g.astype(np.float32))


def _penalty(P, mask, with_sum):
    """sn_param_penalty into buffers filled with NaN."""
    N = P.numel()
    value = torch.full((1,), NAN, dtype=torch.float32, device=P.device)
    grad = torch.full((N,), NAN, dtype=torch.float32, device=P.device)
    with torch.cuda.device(P.device):
        rc = _hip.load().sn_param_penalty(P.data_ptr(), mask.data_ptr(), N, PEN_W, int(with_sum), value.data_ptr(),
                                          grad.data_ptr(), _hip._stream())
    assert rc == 0, _hip.load().sn_last_error()
    return value, grad


@pytest.fixture(scope="module")
def criterion_dense(hip_device):
    """The dense side of the criterion checks: (2, 16385) fp32 predictions through _hip.loss_forward / loss_backward."""
    pred, gt = lc.seeded_inputs((2, 16385), torch.float32, torch.bool)
    pd, gd = pred.to(hip_device), gt.to(hip_device)
    ranges = RANGES10.to(hip_device)
    bin_w = lo.bin_weights(torch.tensor(lc.FREQS), lc.HP["alpha"], lc.HP["eps"], 10).float().to(hip_device)
    loss, stats, coef, loss32 = _hip.loss_forward(pd, gd, ranges, bin_w, WMSE | FOCAL, **CFG)
    up = torch.tensor([0.3], dtype=torch.float32, device=hip_device)
    return dict(pred=pd, gt=gd, ranges=ranges, bin_w=bin_w, loss32=loss32, stats=stats, coef=coef, up=up,
                grad=_grad(pd, gd, ranges, coef, up))


@pytest.mark.parametrize("N", [1, 2, 255, 256, 257, 1000, 4097, 8192])
def test_penalties_at_every_size(hip_device, criterion_dense, N):
    """param_penalty_body stripes N parameters over 256 threads (second trips from 257 on) and keeps 8 N bytes of dynamic
    LDS, 64 KiB at the documented limit of 8192, in its own launch and as the opening of the combine launch.  Value within
    (N / 256 + 16) 2^-24 w sum|terms| of fp64 (strided fp32 partials, four per lane, a 6-level tree), gradient exact."""
    d = criterion_dense
    for over in (False, True):
        Pn, mn = _penalty_inputs(N, over)
        P, mask = torch.from_numpy(Pn).to(hip_device), torch.from_numpy(mn).to(hip_device)
        for with_sum in (False, True):
            want, mag, gwant = _penalty_oracle(Pn, mn, with_sum)
            value, grad = _penalty(P, mask, with_sum)
            bound = (N / 256 + 16) * 2.0 ** -24 * PEN_W * mag
            assert abs(value.item() - want) <= bound, (N, over, with_sum, value.item(), want, bound)
            assert np.array_equal(grad.cpu().numpy(), gwant), (N, over, with_sum)
            assert set(np.unique(gwant)) <= {0.0, -PEN_W, PEN_W}
            # the same work riding in the criterion's two launches
            total, stats, coef, pen_grad = _hip.criterion_forward(d["pred"], d["gt"], d["ranges"], d["bin_w"], WMSE | FOCAL,
                                                                  P, mask, PEN_W, with_sum, **CFG)
            assert torch.equal(total, d["loss32"][0:1] + value)
            assert torch.equal(stats, d["stats"]) and torch.equal(coef, d["coef"])
            assert torch.equal(pen_grad, grad)
            _poison(d["pred"])
            dpred, pen_out = _hip.criterion_backward(d["pred"], d["gt"], d["ranges"], coef, d["up"], pen_grad)
            assert torch.equal(dpred, d["grad"])
            assert torch.equal(pen_out, pen_grad * d["up"])


def test_penalties_refuse_more_than_8192(hip_device, criterion_dense):
    d = criterion_dense
    P = torch.zeros(8193, dtype=torch.float32, device=hip_device)
    mask = torch.ones(8193, dtype=torch.int8, device=hip_device)
    with pytest.raises(sna.HipLibraryError, match=r"sn_param_penalty failed \(-2\)"):       # SN_ERR_UNSUPPORTED
        _hip.param_penalty(P, mask, PEN_W, True)
    with pytest.raises(sna.HipLibraryError, match=r"sn_criterion_forward failed \(-2\)"):
        _hip.criterion_forward(d["pred"], d["gt"], d["ranges"], d["bin_w"], WMSE, P, mask, PEN_W, True)
    assert _hip.device_status()[0] == 0


# ------------------------------------------------------------------ 7. bf16 predictions off 4096 elements
@pytest.mark.parametrize("gt_kind", ["bool", "f32"])
@pytest.mark.parametrize("shape", [(3, 16385), (3, 8196)])
def test_bf16_predictions_in_both_loops(hip_device, shape, gt_kind):
    """The properties of test_criterion_on_bf16_predictions with several backward parts, in the element and in the vector
    loop: the loss is the fp32 loss on the same values (1e-6), the gradient is the fp32 gradient rounded to bf16 bit for
    bit, the loss is within 2e-5 of the fp64 oracle (measured on an MI355X: at most 5.2e-8)."""
    g = torch.Generator().manual_seed(shape[1])
    pred16 = torch.rand(shape, generator=g).clamp(1e-3, 1 - 1e-3).to(torch.bfloat16)
    gtb = torch.rand(shape, generator=g) < 0.1
    gt = gtb if gt_kind == "bool" else torch.where(torch.rand(shape, generator=g) < 0.5, gtb.float(),
                                                   torch.rand(shape, generator=g) * gtb.float())
    loss16, stats16, grad16 = _tversky_case(hip_device, pred16, gt)
    loss32, stats32, grad32 = _tversky_case(hip_device, pred16.float(), gt)
    assert grad16.dtype == torch.bfloat16
    assert abs(loss16 - loss32) <= 1e-6 * abs(loss32)
    assert torch.equal(stats16[:, :10], stats32[:, :10])
    assert torch.equal(grad16, grad32.to(torch.bfloat16))
    ref, _ = lc.tversky_oracle(pred16, gt)
    print(f"bf16 {shape} {gt_kind}: loss error against the oracle {abs(loss16 - ref) / abs(ref):.3g}, tolerance 2e-05")
    assert abs(loss16 - ref) <= 2e-5 * abs(ref)
