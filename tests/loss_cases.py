"""What the criterion tests share (tests/test_gpu_loss.py, tests/test_gpu_loss_plans.py, tests/test_host_logic.py): the
launch plan of K5 restated in Python, and the seeded weighted-MSE + focal-Tversky case with its fp64 oracle.  No test lives
here."""
import torch

import scene_net_amd as sna
from oracle import loss_oracle as lo

# ---------------------------------------------------------------- the launch plan of scene-net_amd/csrc/loss.hip
# forward: SN_LOSS_PARTS(n_per) of include/scenenet_hip.h -- 1 part up to 16384 elements, ceil(n_per / 16384) above,
#   256 from 16384 * 256 on;
# backward: loss.hip:656 -- 1 part up to 8192 elements, ceil(n_per / 8192) above, 512 from 8192 * 512 on;
# span_of (loss.hip:540-544): ceil(n_per / parts) rounded up to a multiple of 4; part q owns [q * span, min((q+1) * span,
#   n_per)); both kernels take the 4-wide loop when n_per % 4 == 0 and the element loop otherwise.
FWD_SPAN, FWD_CAP = 16384, 256
BWD_SPAN, BWD_CAP = 8192, 512


def parts_of(n_per, span, cap):
    return 1 if n_per <= span else (cap if n_per >= span * cap else (n_per + span - 1) // span)


def span_of(n_per, parts):
    return ((n_per + parts - 1) // parts + 3) // 4 * 4


def plan(n_per):
    """(forward parts, forward span, backward parts, backward span, vector loop?)"""
    fp, bp = parts_of(n_per, FWD_SPAN, FWD_CAP), parts_of(n_per, BWD_SPAN, BWD_CAP)
    return fp, span_of(n_per, fp), bp, span_of(n_per, bp), n_per % 4 == 0


def part_bounds(n_per, parts, span):
    """[lo, hi) of every part, as the kernels compute them."""
    return [(q * span, min((q + 1) * span, n_per)) for q in range(parts)]


# n_per of the plan tests: the smallest sizes that reach one part, several parts split exactly and unevenly, and the
# capped part count split exactly and unevenly, in the vector loop and (where a span that is a multiple of 4 allows it) in
# the element loop, on both passes.  SMALL run at B = 3, LARGE at B = 1.
SMALL_N = [8191, 8192, 8193, 8196, 16384, 16385, 16388, 32768]
LARGE_N = [4_194_304, 4_194_307, 4_194_308, 6_000_001]

# ---------------------------------------------------------------- the seeded case: weighted MSE + focal Tversky
FREQS = [3_000_000, 1200, 800, 700, 650, 400, 300, 310, 150, 9000]
HP = dict(alpha=1.5, eps=0.05, mse_weight=2.0)
TVERSKY = dict(tversky_alpha=0.3, tversky_beta=0.7, focal_gamma=2.0, tversky_smooth=0.5)
DTYPE_PAIRS = [(torch.float32, torch.bool), (torch.float32, torch.uint8), (torch.float32, torch.float32),
               (torch.float64, torch.float64), (torch.float32, torch.float64), (torch.float64, torch.float32)]


def oracle_tol(pred_dt):
    """5e-6 for fp32 predictions (the kernels sum in fp64, the gradient arithmetic is fp32), 1e-6 for fp64 ones (the
    oracle's weights' mean is an fp32 reduction); relative to |loss| and to max|grad|."""
    return 5e-6 if pred_dt == torch.float32 else 1e-6


def seeded_inputs(shape, pred_dt, gt_dt):
    """(pred, gt) on the CPU: 5 % ones for byte targets; 90 % zeros, 5 % ones and 5 % values in between for float ones."""
    g = torch.Generator().manual_seed(sum(shape))
    u = torch.rand(shape, generator=g, dtype=torch.float64)
    if gt_dt in (torch.bool, torch.uint8):
        gt = (u < 0.05).to(gt_dt)
    else:
        gt = torch.where(u < 0.9, torch.zeros_like(u), torch.where(u < 0.95, torch.ones_like(u), (u - 0.95) * 20)).to(gt_dt)
    pred = torch.rand(shape, generator=g, dtype=torch.float64).to(pred_dt)
    return pred, gt


def as_oracle_target(gt):
    """Byte targets are float32 to the oracle; float targets keep their dtype (binning happens in it, as in the reference)."""
    return gt.to(torch.float32) if gt.dtype in (torch.bool, torch.uint8) else gt


def tversky_oracle(pred, gt, freqs=FREQS, ranges=None):
    """fp64 oracle of weighted MSE + focal Tversky on the same values: (loss, dloss/dpred) as a float and an fp64 tensor."""
    ranges = torch.linspace(0, 1, 11)[:-1] if ranges is None else ranges
    po = pred.detach().clone().double().requires_grad_(True)
    gto = as_oracle_target(gt)
    w = lo.weight_target(gto, torch.as_tensor(freqs), ranges, HP["alpha"], HP["eps"]).double()
    ref = torch.mean(HP["mse_weight"] * w * (gto.double() - po) ** 2) + \
        lo.focal_tversky_loss(po, gto.double(), TVERSKY["tversky_alpha"], TVERSKY["tversky_beta"], TVERSKY["focal_gamma"],
                              TVERSKY["tversky_smooth"])
    ref.backward()
    return ref.item(), po.grad


def tversky_criterion(dev, freqs=FREQS, ranges=None):
    """sna.GENEO_Tversky_Loss with the hyper-parameters of tversky_oracle."""
    crit = sna.GENEO_Tversky_Loss(targets=torch.zeros(4), weighting_scheme_path=None, save_weighting_scheme=False,
                                  weight_alpha=HP["alpha"], weight_epsilon=HP["eps"], mse_weight=HP["mse_weight"], **TVERSKY)
    crit.freqs = torch.as_tensor(freqs).to(dev)
    if ranges is not None:
        crit.ranges = ranges.to(dev)
    return crit
