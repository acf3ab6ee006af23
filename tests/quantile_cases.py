"""What the quantile-loss tests share (tests/test_quantile_host.py, tests/test_gpu_quantile_loss.py,
tests/golden/make_golden_quantile.py): the launch plan of K20 restated in Python, the seeded inputs with planted ties, and
the fp64 oracle of the weighted pinball loss.  No test lives here."""
import os

import numpy as np
import torch

import loss_cases as lc
from oracle import loss_oracle as lo

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "quantile_loss.npz")

# ---------------------------------------------------------------- the launch plan of scene-net_amd/csrc/quantile.hip
# K5's own (include/scenenet_hip.h: SN_QUANTILE_PARTS = SN_LOSS_PARTS, SN_QUANTILE_BWD_PARTS): forward 1 part up to 16384
# voxels, ceil(n_per / 16384) above, 256 from 16384 * 256 on; backward 1 part up to 8192, ceil(n_per / 8192) above, 512 from
# 8192 * 512 on; a part spans ceil(n_per / parts) voxels rounded up to a multiple of 4; both kernels take the 4-wide loop
# when n_per % 4 == 0 and the element loop otherwise.  A voxel's Q channels belong to the part that owns the voxel.
FWD_SPAN, FWD_CAP, BWD_SPAN, BWD_CAP = lc.FWD_SPAN, lc.FWD_CAP, lc.BWD_SPAN, lc.BWD_CAP
MAX_Q = 8


def plan(n_per):
    """(forward parts, forward span, backward parts, backward span, vector loop?)"""
    return lc.plan(n_per)


# one part on both passes / two backward parts split exactly / unevenly in the element and the vector loop / two forward
# parts split exactly / unevenly in the element and the vector loop / four backward parts
PLAN_N = [8191, 8192, 8193, 8196, 16384, 16385, 16388, 32768]
CAPPED_N = 4_194_307   # 256 forward and 512 backward parts, uneven, element loop

# ---------------------------------------------------------------- the seeded case
FREQS = lc.FREQS
HP = dict(alpha=1.5, epsilon=0.05)
QS = {1: [0.5], 2: [0.25, 0.8], 3: [0.1, 0.5, 0.9], 8: [0.05, 0.1, 0.25, 0.4, 0.5, 0.6, 0.75, 0.95]}


def seeded_inputs(B, Q, spatial, pred_dt, gt_dt, tie_fraction=1.0 / 3):
    """(pred [B, Q, *spatial], gt [B, *spatial]) on the CPU: loss_cases.seeded_inputs' targets (90 % zeros for float ones)
    and uniform predictions, of which `tie_fraction` are overwritten by their voxel's target -- exact ties wherever the
    target is representable in pred's dtype (every zero and one is)."""
    spatial = tuple(spatial)
    _, gt = lc.seeded_inputs((B,) + spatial, pred_dt, gt_dt)
    g = torch.Generator().manual_seed(1000 * Q + B + sum(spatial))
    pred = torch.rand((B, Q) + spatial, generator=g, dtype=torch.float64).to(pred_dt)
    tie = torch.rand((B, Q) + spatial, generator=g, dtype=torch.float64) < tie_fraction
    gt_b = gt.to(pred_dt).unsqueeze(1).expand(pred.shape)
    return torch.where(tie, gt_b, pred).contiguous(), gt


def q_pairs(qs):
    """(q_i, q_i - 1) as fp64 values of the float32 numbers the reference forms (quant_loss.py:57-58, :86)."""
    q32 = torch.as_tensor(qs, dtype=torch.float32).reshape(-1)
    return q32.double(), (q32 - 1).double()


def pinball_sum(pred64, gt64, qs):
    """sum_i max(q_i d, (q_i - 1) d), d = gt - pred[:, i]: [B, ...] from pred [B, Q, ...] and gt [B, ...], fp64."""
    q, qm1 = q_pairs(qs)
    out = 0
    for i in range(len(q)):
        d = gt64 - pred64[:, i]
        out = out + torch.max(q[i] * d, qm1[i] * d)
    return out


def raw_weights(gt, freqs=FREQS, ranges=None, alpha=HP["alpha"], eps=HP["epsilon"]):
    """bin_w at the target's bin, before the division by the mean (fp32, as the reference holds them)."""
    ranges = torch.linspace(0, 1, 11)[:-1] if ranges is None else ranges
    gto = lc.as_oracle_target(gt)
    return lo.bin_weights(torch.as_tensor(freqs), alpha, eps, len(ranges))[lo.nearest_bin(gto, ranges)]


def oracle(pred, gt, qs, freqs=FREQS, ranges=None, alpha=HP["alpha"], eps=HP["epsilon"]):
    """fp64 oracle, per sample: (loss, dloss/dpred fp64, shares [Q] fp64).  Weights: oracle.loss_oracle.weight_target."""
    ranges = torch.linspace(0, 1, 11)[:-1] if ranges is None else ranges
    gt = gt.reshape((pred.shape[0],) + tuple(pred.shape[2:]))
    gto = lc.as_oracle_target(gt)
    w = lo.weight_target(gto, torch.as_tensor(freqs), ranges, alpha, eps).double()
    po = pred.detach().clone().double().requires_grad_(True)
    q, qm1 = q_pairs(qs)
    shares = []
    for i in range(len(q)):
        d = gto.double() - po[:, i]
        shares.append(torch.mean(w * torch.max(q[i] * d, qm1[i] * d)))
    loss = sum(shares)
    loss.backward()
    return loss.item(), po.grad, torch.stack(shares).detach()


def criterion(sna, dev, qs, freqs=FREQS, ranges=None, cls=None, **kw):
    """sna.QuantileLoss (or `cls`) with the hyper-parameters of `oracle`."""
    cls = sna.QuantileLoss if cls is None else cls
    crit = cls(targets=torch.zeros(4), qs=torch.tensor(qs), hist_path=None, save_weighting_scheme=False,
               alpha=HP["alpha"], epsilon=HP["epsilon"], **kw)
    crit.freqs = torch.as_tensor(freqs).to(dev)
    if ranges is not None:
        crit.ranges = ranges.to(dev)
    return crit


def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


# ---------------------------------------------------------------- the golden inputs (tests/golden/make_golden_quantile.py)
GOLDEN_QS = [0.1, 0.5, 0.9]
GOLDEN_HP = dict(alpha=1.0, epsilon=0.1)


def golden_inputs(B):
    """pred [B, 3, 6, 6, 6] f32 and gt [B, 1, 6, 6, 6] f32 (ratio-like targets; a third of the predictions tie)."""
    pred, gt = seeded_inputs(B, 3, (6, 6, 6), torch.float32, torch.float32)
    return pred, gt.unsqueeze(1).contiguous()


def golden_pair():
    """(inputs in (0, 1), binary float targets), [2, 1, 6, 6, 6] f32: the FocalLoss / IoULoss pair."""
    g = torch.Generator().manual_seed(77)
    p = torch.rand((2, 1, 6, 6, 6), generator=g, dtype=torch.float64).clamp(1e-3, 1 - 1e-3).to(torch.float32)
    t = (torch.rand((2, 1, 6, 6, 6), generator=g, dtype=torch.float64) < 0.2).to(torch.float32)
    return p, t
