"""The weighted pinball loss without a GPU: the fp64 oracle of tests/quantile_cases.py against the reference's own numbers
(tests/golden/quantile_loss.npz), what the reference's broadcast computes at B = 2, the argument checks of
sn_quantile_forward / sn_quantile_backward, the refusal of CPU tensors and the launch plan against the header's macros."""
import ctypes
import os
import re

import pytest
import torch

import scene_net_amd as sna
from scene_net_amd import _hip
import quantile_cases as qc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the tolerance tests/test_gpu_loss.py gives the reference's float32 reductions
REF_TOL = 2e-5


@pytest.fixture(scope="module")
def gold():
    return qc.golden()


def _oracle_of(gold, B, pred=None, gt=None):
    pred = torch.from_numpy(gold[f"b{B}|pred"]) if pred is None else pred
    gt = torch.from_numpy(gold[f"b{B}|gt"]) if gt is None else gt
    alpha, eps = gold["hp"]
    return qc.oracle(pred, gt, gold["qs"], freqs=torch.from_numpy(gold[f"b{B}|freqs"]),
                     ranges=torch.from_numpy(gold[f"b{B}|ranges"]), alpha=float(alpha), eps=float(eps))


def test_golden_inputs_hold_planted_ties(gold):
    pred, gt = torch.from_numpy(gold["b1|pred"]), torch.from_numpy(gold["b1|gt"])
    assert pred.shape == (1, 3, 6, 6, 6) and gt.shape == (1, 1, 6, 6, 6) and pred.dtype == gt.dtype == torch.float32
    ties = pred == gt
    assert 0.25 < ties.float().mean().item() < 0.42          # a third of the predictions tie ...
    assert (ties & (gt == 0)).sum().item() > 100               # ... zeros among them, where the model's relu sits
    assert (ties & (gt != 0)).sum().item() > 0


def test_oracle_reproduces_the_reference_at_b1(gold):
    loss, grad, shares = _oracle_of(gold, 1)
    ref_loss, ref_grad = float(gold["b1|loss"]), torch.from_numpy(gold["b1|grad"]).double()
    print(f"loss {loss:.9g} reference {ref_loss:.9g}; max |grad diff| {(grad - ref_grad).abs().max().item():.3g} of "
          f"{ref_grad.abs().max().item():.3g}")
    assert abs(loss - ref_loss) <= REF_TOL * abs(ref_loss)
    assert (grad - ref_grad).abs().max().item() <= REF_TOL * ref_grad.abs().max().item()
    assert abs(shares.sum().item() - loss) <= 1e-12 * abs(loss)
    # the unweighted per-voxel sum is the reference's quantile_loss
    pred, gt = torch.from_numpy(gold["b1|pred"]), torch.from_numpy(gold["b1|gt"])
    mine = qc.pinball_sum(pred.double(), gt[:, 0].double(), gold["qs"])
    ref = torch.from_numpy(gold["b1|quantile_loss"]).double()[:, 0]
    assert (mine - ref).abs().max().item() <= REF_TOL * ref.abs().max().item()


def test_reference_broadcast_at_b2_is_every_pair(gold):
    """quantile_loss of the reference at B = 2 is [2, 2, ...]: entry [a, b] pairs gt[a] with pred[b].  The per-sample
    loss is the diagonal; the reference's scalar is the mean over all four pairs."""
    pred, gt = torch.from_numpy(gold["b2|pred"]), torch.from_numpy(gold["b2|gt"])
    ref = torch.from_numpy(gold["b2|quantile_loss"]).double()
    assert tuple(ref.shape) == (2, 2, 6, 6, 6)
    for a in range(2):
        for b in range(2):
            mine = qc.pinball_sum(pred[b:b + 1].double(), gt[a:a + 1, 0].double(), gold["qs"])[0]
            assert (mine - ref[a, b]).abs().max().item() <= REF_TOL * ref.abs().max().item()
    w = torch.from_numpy(gold["b2|weights"]).double()          # [2, 1, ...], mean 1 over both samples
    cross = torch.mean(w * ref).item()
    assert abs(cross - float(gold["b2|loss"])) <= REF_TOL * abs(cross)
    per_sample = torch.mean(w[:, 0] * torch.stack([ref[0, 0], ref[1, 1]])).item()
    loss, _, _ = _oracle_of(gold, 2)
    assert abs(loss - per_sample) <= REF_TOL * abs(per_sample)
    assert abs(loss - cross) > 1e-3 * abs(cross)               # ... and it is not the mean over all pairs


def test_argument_checks_need_no_gpu():
    lib = _hip.load()
    buf = ctypes.create_string_buffer(4096 + 64)
    base = (ctypes.addressof(buf) + 63) // 64 * 64
    p = ctypes.c_void_p(base)
    qs = (ctypes.c_float * 8)(0.1, 0.5, 0.9, 0.5, 0.5, 0.5, 0.5, 0.5)
    q = ctypes.cast(qs, ctypes.c_void_p)

    def fwd(pred=p, pdt=_hip.SN_F32, gt=p, gdt=_hip.SN_F32, B=1, Q=3, n=8, qs_=q, ranges=p, bw=p, H=10, ws=p, stats=p,
            loss=p, coef=p):
        return lib.sn_quantile_forward(pred, pdt, gt, gdt, B, Q, n, qs_, ranges, bw, H, ws, stats, loss, None, coef, None)

    def bwd(pred=p, pdt=_hip.SN_F32, gt=p, gdt=_hip.SN_F32, B=1, Q=3, n=8, qs_=q, ranges=p, H=10, coef=p, grad=p):
        return lib.sn_quantile_backward(pred, pdt, gt, gdt, B, Q, n, qs_, ranges, H, coef, None, _hip.SN_F64, grad, None)

    for call in (fwd, bwd):
        for kw in (dict(pred=None), dict(gt=None), dict(qs_=None), dict(ranges=None), dict(coef=None)):
            assert call(**kw) == -1, kw
            assert b"null" in lib.sn_last_error()
        for kw in (dict(B=0), dict(B=-2), dict(n=0), dict(Q=0), dict(Q=9), dict(H=0), dict(H=_hip.SN_LOSS_MAX_BINS + 1)):
            assert call(**kw) == -1, kw
            assert lib.sn_last_error()
        assert call(pdt=_hip.SN_BF16) == -2
        assert b"bf16" in lib.sn_last_error()
        for bad in (0.0, 1.0, -0.2, 1.5, float("nan")):
            bad_qs = (ctypes.c_float * 3)(0.1, bad, 0.9)
            assert call(qs_=ctypes.cast(bad_qs, ctypes.c_void_p)) == -2, bad
            assert b"quantile 1" in lib.sn_last_error()
    assert fwd(bw=None) == -1 and fwd(ws=None) == -1 and fwd(stats=None) == -1 and fwd(loss=None) == -1
    assert bwd(grad=None) == -1


def test_cpu_tensors_raise():
    crit = qc.criterion(sna, "cpu", qc.QS[3])
    pred, gt = qc.seeded_inputs(1, 3, (4, 4, 4), torch.float32, torch.float32)
    with pytest.raises(sna.HipLibraryError):
        crit(pred, gt)
    with pytest.raises(sna.HipLibraryError):
        crit.quantile_loss(pred, gt)
    geneo = qc.criterion(sna, "cpu", qc.QS[3], cls=sna.QuantileGENEOLoss)
    with pytest.raises(sna.HipLibraryError):
        geneo(pred, gt, [], [])
    p, t = qc.golden_pair()
    for crit2 in (sna.FocalLoss("mean"), sna.FocalLoss("none"), sna.IoULoss()):
        with pytest.raises(sna.HipLibraryError):
            crit2(p, t)


def test_constructor_is_the_reference_signature_made_to_work():
    crit = sna.QuantileGENEOLoss(torch.rand(64), torch.tensor([0.2, 0.7]), None, 2.0, 3.0, 0.05, 4.0,
                                 save_weighting_scheme=False)
    assert (crit.weight_alpha, crit.cvx_w, crit.weight_epsilon, crit.gamma) == (2.0, 3.0, 0.05, 4.0)
    assert tuple(crit.qs.shape) == (2, 1) and crit.qs.dtype == torch.float32
    assert torch.equal(crit._qs.cpu(), torch.tensor([[0.2, 0.2 - 1], [0.7, 0.7 - 1]], dtype=torch.float32))
    for bad in ([0.0, 0.5], [0.5, 1.0], [-0.1]):
        with pytest.raises(AssertionError):
            sna.QuantileLoss(torch.rand(8), torch.tensor(bad), None, save_weighting_scheme=False)
    import argparse
    parser = sna.FocalLoss.add_model_specific_args(argparse.ArgumentParser())
    ns = parser.parse_args([])
    assert (ns.focal_alpha, ns.focal_gamma) == (0.5, 2)


def _macro(src, name):
    m = re.search(r"#define\s+" + name + r"\(([^)]*)\)\s+(.*)", src)
    assert m, name
    return m.group(2).split("/*")[0].strip()


def test_plan_helper_matches_the_header():
    src = open(os.path.join(ROOT, "include", "scenenet_hip.h")).read()
    assert _macro(src, "SN_QUANTILE_PARTS") == "SN_LOSS_PARTS(n_per)"
    assert _macro(src, "SN_LOSS_PARTS") == \
        "((n_per) <= 16384 ? 1 : ((n_per) >= 16384 * 256 ? 256 : (int)(((n_per) + 16383) / 16384)))"
    assert _macro(src, "SN_QUANTILE_BWD_PARTS") == \
        "((n_per) <= 8192 ? 1 : ((n_per) >= 8192 * 512 ? 512 : (int)(((n_per) + 8191) / 8192)))"
    assert re.search(r"#define\s+SN_QUANTILE_MAX_Q\s+8\b", src) and qc.MAX_Q == _hip.SN_QUANTILE_MAX_Q == 8
    assert (qc.FWD_SPAN, qc.FWD_CAP, qc.BWD_SPAN, qc.BWD_CAP) == (16384, 256, 8192, 512)
    for n in qc.PLAN_N + [1, 3, 16383, qc.CAPPED_N, 8192 * 512 - 1, 8192 * 512, 16384 * 256 - 1, 16384 * 256, 10 ** 9]:
        fp, fspan, bp, bspan, _ = qc.plan(n)
        assert (fp, bp) == _hip.quantile_parts(n), n
        assert fspan % 4 == 0 and bspan % 4 == 0 and fp * fspan >= n and bp * bspan >= n
    # the sizes of the GPU test reach what they are there for
    assert [qc.plan(n)[0] for n in qc.PLAN_N] == [1, 1, 1, 1, 1, 2, 2, 2]
    assert [qc.plan(n)[2] for n in qc.PLAN_N] == [1, 1, 2, 2, 2, 3, 3, 4]
    assert [qc.plan(n)[4] for n in qc.PLAN_N] == [False, True, False, True, True, False, True, True]
    assert qc.plan(qc.CAPPED_N)[0] == 256 and qc.plan(qc.CAPPED_N)[2] == 512
