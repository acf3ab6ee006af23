"""K20 on the GPU: sna.QuantileLoss / QuantileGENEOLoss (csrc/quantile.hip) against the reference's own numbers at B = 1
(tests/golden/quantile_loss.npz) and against the fp64 oracle of tests/quantile_cases.py at every boundary of the launch
plan, every dtype pair and Q in {1, 3, 8}; ties, the per-sample rule, shapes, upstream scalars, determinism, the ensemble,
graph capture; FocalLoss and IoULoss against their goldens."""
import functools

import pytest
import torch

import scene_net_amd as sna
import loss_cases as lc
import quantile_cases as qc

pytestmark = pytest.mark.gpu

REF_TOL = 2e-5   # what tests/test_gpu_loss.py gives the reference's float32 reductions


@functools.lru_cache(maxsize=None)
def _gold():
    return qc.golden()


def _run(crit, pred_cpu, gt_cpu, dev, scale=None):
    """(loss tensor, grad, shares) of one forward + backward on the device."""
    pred = pred_cpu.to(dev).requires_grad_(True)
    loss = crit(pred, gt_cpu.to(dev))
    shares = crit.last_quantile_terms
    (loss if scale is None else scale(loss)).backward()
    return loss.detach(), pred.grad, shares


def _check(loss, grad, ref_loss, ref_grad, tol, what=""):
    gmax = ref_grad.abs().max().item()
    le = abs(loss.double().item() - ref_loss) / abs(ref_loss)
    ge = (grad.double().cpu() - ref_grad).abs().max().item() / gmax
    print(f"{what}: loss {loss.double().item():.12g} ref {ref_loss:.12g} rel {le:.3g}; grad rel {ge:.3g} (tol {tol:g})")
    assert le <= tol, what
    assert ge <= tol, what


# ---------------------------------------------------------------- 1. golden
def test_golden_b1(hip_device):
    z = _gold()
    alpha, eps = z["hp"]
    crit = sna.QuantileLoss(targets=torch.zeros(4), qs=torch.from_numpy(z["qs"]), hist_path=None, alpha=float(alpha),
                            epsilon=float(eps), save_weighting_scheme=False)
    crit.freqs, crit.ranges = torch.from_numpy(z["b1|freqs"]).to(hip_device), torch.from_numpy(z["b1|ranges"]).to(hip_device)
    pred, gt = torch.from_numpy(z["b1|pred"]), torch.from_numpy(z["b1|gt"])
    loss, grad, _ = _run(crit, pred, gt, hip_device)
    assert loss.dtype == torch.float32 and loss.dim() == 0
    _check(loss, grad, float(z["b1|loss"]), torch.from_numpy(z["b1|grad"]).double(), REF_TOL, "golden")
    # quantile_loss: the reference's method, per sample
    ql = crit.quantile_loss(pred.to(hip_device), gt.to(hip_device)).cpu()
    ref = torch.from_numpy(z["b1|quantile_loss"])[:, 0]
    assert ql.shape == ref.shape and (ql - ref).abs().max().item() <= REF_TOL * ref.abs().max().item()


# ---------------------------------------------------------------- 2. oracle parity
@pytest.mark.parametrize("Q", [1, 3, 8])
@pytest.mark.parametrize("pred_dt,gt_dt", lc.DTYPE_PAIRS, ids=lambda d: str(d).replace("torch.", ""))
def test_oracle_parity_at_the_plan_boundaries(hip_device, pred_dt, gt_dt, Q):
    crit = qc.criterion(sna, hip_device, qc.QS[Q])
    for n_per in qc.PLAN_N:
        pred, gt = qc.seeded_inputs(2, Q, (n_per,), pred_dt, gt_dt)
        ref_loss, ref_grad, ref_shares = qc.oracle(pred, gt, qc.QS[Q])
        loss, grad, shares = _run(crit, pred, gt, hip_device)
        assert loss.dtype == pred_dt and grad.dtype == pred_dt and grad.shape == pred.shape
        _check(loss, grad, ref_loss, ref_grad, lc.oracle_tol(pred_dt), f"n_per {n_per} Q {Q}")
        assert (shares.cpu() - ref_shares).abs().max().item() <= lc.oracle_tol(pred_dt) * abs(ref_loss)


def test_oracle_parity_at_the_capped_part_counts(hip_device):
    assert qc.plan(qc.CAPPED_N)[0] == qc.FWD_CAP and qc.plan(qc.CAPPED_N)[2] == qc.BWD_CAP
    crit = qc.criterion(sna, hip_device, qc.QS[2])
    pred, gt = qc.seeded_inputs(1, 2, (qc.CAPPED_N,), torch.float32, torch.float32)
    ref_loss, ref_grad, _ = qc.oracle(pred, gt, qc.QS[2])
    loss, grad, _ = _run(crit, pred, gt, hip_device)
    _check(loss, grad, ref_loss, ref_grad, lc.oracle_tol(torch.float32), "capped")


# ---------------------------------------------------------------- 3. ties
@pytest.mark.parametrize("dt", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_ties_and_the_smallest_step_either_side(hip_device, dt):
    qs = qc.QS[3]
    n = 4 * 1031
    values = torch.tensor([0.0, 1.0, 0.3, 0.625], dtype=dt)
    gt = values[torch.arange(n) % 4].reshape(1, n)
    up_ = torch.nextafter(gt, torch.full_like(gt, 2.0))
    down = torch.nextafter(gt, torch.full_like(gt, -2.0))
    # channel i, voxel v: tie / pred one step above gt (d < 0) / one step below (d > 0), shifted by the channel
    kind = (torch.arange(n).reshape(1, n) // 4 + torch.arange(3).reshape(3, 1)) % 3
    pred = torch.where(kind == 0, gt, torch.where(kind == 1, up_, down)).reshape(1, 3, n).contiguous()
    assert (pred[0][kind == 0] == gt.expand(3, n)[kind == 0]).all() and (pred[0][kind == 1] > gt.expand(3, n)[kind == 1]).all()
    crit = qc.criterion(sna, hip_device, qs)
    _, grad, _ = _run(crit, pred, gt, hip_device, scale=lambda l: 2.5 * l)
    w = qc.raw_weights(gt).double()
    coef = (w / w.sum()).expand(3, n)
    q = torch.tensor(qs, dtype=torch.float32).double().reshape(3, 1)
    g = torch.where(kind == 0, 0.5 - q, torch.where(kind == 1, 1 - q, -q))
    want = (2.5 * coef * g).reshape(1, 3, n)
    err = (grad.double().cpu() - want).abs().max().item() / want.abs().max().item()
    print(f"ties {dt}: grad rel {err:.3g}")
    assert err <= lc.oracle_tol(dt)
    # the three cases are told apart exactly: a tie never takes a side's value
    got = grad.double().cpu()[0] / (2.5 * coef)
    assert ((got - g).abs() < 0.01).all()


# ---------------------------------------------------------------- 4. per sample
def test_per_sample_not_the_cross_broadcast(hip_device):
    qs = qc.QS[3]
    pred, gt = qc.seeded_inputs(3, 3, (6, 6, 6), torch.float32, torch.float32)
    assert not torch.equal(gt[0], gt[1]) and not torch.equal(pred[0], pred[2])
    ref_loss, ref_grad, _ = qc.oracle(pred, gt, qs)
    loss, grad, _ = _run(qc.criterion(sna, hip_device, qs), pred, gt, hip_device)
    _check(loss, grad, ref_loss, ref_grad, lc.oracle_tol(torch.float32), "per sample")
    w = qc.raw_weights(gt).double()
    w = w / w.mean()
    cross = torch.stack([w[a] * qc.pinball_sum(pred[b:b + 1].double(), gt[a:a + 1].double(), qs)[0]
                         for a in range(3) for b in range(3)]).mean().item()
    assert abs(loss.item() - cross) > 1e-3 * abs(cross)


# ---------------------------------------------------------------- 5. shapes
def test_target_shapes_and_strided_predictions(hip_device):
    qs = qc.QS[3]
    crit = qc.criterion(sna, hip_device, qs)
    pred, gt = qc.seeded_inputs(2, 3, (6, 10, 12), torch.float32, torch.float32)
    l0, g0, s0 = _run(crit, pred, gt, hip_device)
    l1, g1, s1 = _run(crit, pred, gt.unsqueeze(1), hip_device)
    assert torch.equal(l0, l1) and torch.equal(g0, g1) and torch.equal(s0, s1)
    strided = pred.permute(0, 2, 3, 4, 1).contiguous().to(hip_device).permute(0, 4, 1, 2, 3).requires_grad_(True)
    assert not strided.is_contiguous() and torch.equal(strided.detach().cpu(), pred)
    l2 = crit(strided, gt.to(hip_device))
    l2.backward()
    assert torch.equal(l2.detach(), l0) and torch.equal(strided.grad, g0)


# ---------------------------------------------------------------- 6. Q = 1
def test_median_is_half_the_weighted_l1(hip_device):
    pred, gt = qc.seeded_inputs(2, 1, (8193,), torch.float32, torch.float32)
    w = qc.raw_weights(gt).double()
    l1 = torch.mean(w / w.mean() * (gt.double() - pred[:, 0].double()).abs()).item()
    loss, _, shares = _run(qc.criterion(sna, hip_device, [0.5]), pred, gt, hip_device)
    assert abs(loss.item() - 0.5 * l1) <= lc.oracle_tol(torch.float32) * 0.5 * l1
    assert shares.shape == (1,) and abs(shares.item() - 0.5 * l1) <= lc.oracle_tol(torch.float32) * 0.5 * l1


# ---------------------------------------------------------------- 7. upstream and determinism
@pytest.mark.parametrize("dt", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_upstream_scalar_and_determinism(hip_device, dt):
    qs = qc.QS[3]
    crit = qc.criterion(sna, hip_device, qs)
    pred, gt = qc.seeded_inputs(2, 3, (16388,), dt, torch.float32)
    l0, g0, s0 = _run(crit, pred, gt, hip_device)
    l1, g1, s1 = _run(crit, pred, gt, hip_device)
    assert torch.equal(l0, l1) and torch.equal(g0, g1) and torch.equal(s0, s1)
    assert s0.dtype == torch.float64 and not s0.requires_grad
    total = s0.sum().item()
    l64 = l0.double().item()
    if dt == torch.float64:
        assert abs(total - l64) <= 1e-12 * abs(l64)
    else:   # the float32 scalar is the fp64 total rounded once
        assert abs(total - l64) <= 2.0 ** -24 * abs(l64) * 1.0001
    _, g3, _ = _run(crit, pred, gt, hip_device, scale=lambda l: 3 * l)            # upstream in pred's dtype
    assert (g3.double() - 3 * g0.double()).abs().max().item() <= lc.oracle_tol(dt) * 3 * g0.abs().max().item()
    _, g3d, _ = _run(crit, pred, gt, hip_device, scale=lambda l: 3 * l.double())  # through a cast node
    assert (g3d.double() - 3 * g0.double()).abs().max().item() <= lc.oracle_tol(dt) * 3 * g0.abs().max().item()


def test_shares_sum_to_the_total(hip_device):
    from scene_net_amd import _hip
    crit = qc.criterion(sna, hip_device, qc.QS[8])
    pred, gt = qc.seeded_inputs(2, 8, (16385,), torch.float32, torch.bool)
    ranges, bin_w = crit._device_tables(hip_device)
    loss, loss32, stats, coef = _hip.quantile_forward(pred.to(hip_device), gt.to(hip_device), crit._qs_host, ranges, bin_w)
    assert abs(loss[1:].sum().item() - loss[0].item()) <= 1e-12 * abs(loss[0].item())
    assert torch.equal(loss32, loss.float())
    H = ranges.numel()
    counts = stats[:, 8:].sum(0).cpu()
    assert counts.sum().item() == 2 * 16385 and counts[0].item() == (~gt).sum().item()
    assert stats.shape == (2, 8 + H) and coef.shape == (H,)
    w = qc.raw_weights(gt).double()
    assert abs(coef[0].item() - (w[~gt][0] / w.sum()).item()) <= 1e-12


# ---------------------------------------------------------------- 8. the ensemble
def test_quantile_geneo_loss_trains_the_ensemble(hip_device):
    torch.manual_seed(11)
    qs = torch.tensor(qc.QS[3])
    ks = (9, 5, 5)   # tests/test_gpu_training.py: the smallest kernel its differentiable forward runs
    model = sna.SCENENetQuantile({"cy": 1, "cone": 1, "neg": 1}, ks, qs=qs).to(hip_device)
    with torch.no_grad():
        for net in model.scnets:
            for n in net.geneos:
                net.lambdas_dict[f"lambda_{n}"].mul_(0.1)
        for net in model.scnets[:2]:   # a negative trainable coefficient: the penalties are live
            free = [k for k in net.lambdas_dict if k != net.last_lambda][0]
            net.lambdas_dict[free].fill_(-0.05)
    g = torch.Generator().manual_seed(5)
    x = (torch.rand((2, 1, 16, 16, 16), generator=g) < 0.2).to(hip_device)
    y = (torch.rand((2, 1, 16, 16, 16), generator=g) < 0.05).to(hip_device)
    crit = sna.QuantileGENEOLoss(targets=y.float(), qs=qs, hist_path=None, rho=2.0, save_weighting_scheme=False)
    params = [p for p in model.parameters() if p.requires_grad]

    def grads(criterion_of):
        for p in params:
            p.grad = None
        pred = model(x)
        assert pred.shape == (2, 3, 16, 16, 16) and pred.dtype == torch.float32
        cvx, gp = model.get_cvx_coefficients(), model.get_geneo_params()
        loss = criterion_of(pred) + crit.cvx_loss(cvx) + crit.positive_regularizer(gp)
        loss.backward()
        return loss.item(), [torch.zeros(()) if p.grad is None else p.grad.detach().cpu().clone() for p in params]

    def restated(pred):   # the criterion alone replaced by torch ops on the same predictions
        w = crit.get_weight_target(y.float())
        return torch.mean(w * crit.quantile_loss(pred, y).unsqueeze(1))

    pred = model(x)
    cvx, gp = model.get_cvx_coefficients(), model.get_geneo_params()
    full = crit(pred, y, cvx, gp)
    penalty = crit.cvx_loss(cvx) + crit.positive_regularizer(gp)
    per_net = sum(sna.GENEO_Loss.cvx_loss(crit, {k: v for k, v in c.items()}) for c in cvx) + \
        sum(sna.GENEO_Loss.positive_regularizer(crit, {k: v for k, v in p_.items()}) for p_ in gp)
    assert penalty.item() > 0 and abs(penalty.item() - per_net.item()) <= 1e-6
    dense = sna.QuantileLoss.forward(crit, pred, y)
    assert abs(full.item() - (dense.item() + penalty.item())) <= 1e-6
    del pred, full, dense, penalty, per_net

    l_hip, g_hip = grads(lambda pred: sna.QuantileLoss.forward(crit, pred, y))
    l_ref, g_ref = grads(restated)
    assert abs(l_hip - l_ref) <= REF_TOL * abs(l_ref)
    biggest = max(gr.abs().max().item() for gr in g_ref)
    assert biggest > 0
    worst = max((a - b).abs().max().item() for a, b in zip(g_hip, g_ref))
    print(f"ensemble: loss {l_hip:.9g} / {l_ref:.9g}; worst grad diff {worst:.3g} of {biggest:.3g}")
    assert worst <= lc.oracle_tol(torch.float32) * biggest


# ---------------------------------------------------------------- 9. capture
def test_forward_and_backward_replay_from_a_graph(hip_device):
    qs = qc.QS[3]
    crit = qc.criterion(sna, hip_device, qs)
    pred_a, gt_a = qc.seeded_inputs(2, 3, (16388,), torch.float32, torch.float32)
    pred_b, gt_b = qc.seeded_inputs(2, 3, (16388,), torch.float32, torch.float32, tie_fraction=0.5)
    pred_b = (pred_b * 0.5).contiguous()
    assert not torch.equal(pred_a, pred_b)
    pred_s = pred_a.to(hip_device).requires_grad_(True)
    gt_s = gt_a.to(hip_device)

    def step():
        loss = crit(pred_s, gt_s)
        (grad,) = torch.autograd.grad(loss, pred_s)
        return loss, grad, crit.last_quantile_terms

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss_g, grad_g, shares_g = step()
    for pred_x, gt_x in ((pred_b, gt_b), (pred_a, gt_a)):
        with torch.no_grad():
            pred_s.copy_(pred_x.to(hip_device))
            gt_s.copy_(gt_x.to(hip_device))
        graph.replay()
        torch.cuda.synchronize()
        loss_e, grad_e, shares_e = _run(crit, pred_x, gt_x, hip_device)
        assert torch.equal(loss_g, loss_e) and torch.equal(grad_g, grad_e) and torch.equal(shares_g, shares_e)


# ---------------------------------------------------------------- 10. FocalLoss / IoULoss
@pytest.mark.parametrize("reduction", ["mean", "sum", "none"])
def test_focal_loss_golden(hip_device, reduction):
    z = _gold()
    p = torch.from_numpy(z["pair|inputs"]).to(hip_device).requires_grad_(True)
    t = torch.from_numpy(z["pair|targets"]).to(hip_device)
    crit = sna.FocalLoss(reduction=reduction, alpha=float(z["pair|focal_alpha"]), gamma=float(z["pair|focal_gamma"]))
    loss = crit(p, t)
    loss.sum().backward()
    ref_l, ref_g = torch.from_numpy(z[f"pair|focal_{reduction}|loss"]), torch.from_numpy(z[f"pair|focal_{reduction}|grad"])
    assert loss.shape == ref_l.shape
    assert (loss.detach().cpu() - ref_l).abs().max().item() <= REF_TOL * ref_l.abs().max().item()
    assert (p.grad.cpu() - ref_g).abs().max().item() <= REF_TOL * ref_g.abs().max().item()


@pytest.mark.parametrize("smooth", [1, 0.5])
def test_iou_loss_golden_and_is_tversky(hip_device, smooth):
    z = _gold()
    t = torch.from_numpy(z["pair|targets"]).to(hip_device)
    out = []
    for crit in (lambda a, b: sna.IoULoss()(a, b, smooth=smooth), sna.TverskyLoss(1, 1, smooth)):
        p = torch.from_numpy(z["pair|inputs"]).to(hip_device).requires_grad_(True)
        loss = crit(p, t)
        loss.backward()
        out.append((loss.detach(), p.grad))
    (l_iou, g_iou), (l_tv, g_tv) = out
    assert torch.equal(l_iou, l_tv) and torch.equal(g_iou, g_tv)
    ref_l, ref_g = float(z[f"pair|iou_{smooth}|loss"]), torch.from_numpy(z[f"pair|iou_{smooth}|grad"])
    assert abs(l_iou.item() - ref_l) <= REF_TOL * abs(ref_l)
    assert (g_iou.cpu() - ref_g).abs().max().item() <= REF_TOL * ref_g.abs().max().item()


# ---------------------------------------------------------------- 11. NaN
def test_nan_prediction_gives_nan_loss(hip_device):
    pred, gt = qc.seeded_inputs(2, 3, (8196,), torch.float32, torch.float32)
    pred[1, 2, 4321] = float("nan")
    crit = qc.criterion(sna, hip_device, qc.QS[3])
    loss = crit(pred.to(hip_device), gt.to(hip_device))
    assert torch.isnan(loss).item()
    assert torch.isnan(crit.last_quantile_terms[2]).item() and not torch.isnan(crit.last_quantile_terms[0]).item()
