"""
Generates tests/golden/quantile_loss.npz by IMPORTING the reference (dlavado/scene-net) where it is checked out
(SCENENET_REFERENCE) and running its own QuantileLoss (core/criterions/quant_loss.py), FocalLoss (focal_loss.py) and
IoULoss (iou_loss.py) on the inputs of tests/quantile_cases.py.  The reference never travels: only the inputs and the arrays
it returned are committed.  Run from the repo root:

    SCENENET_REFERENCE=<checkout of the reference> python tests/golden/make_golden_quantile.py

Third-party modules the reference imports for plotting / IO only are replaced by MagicMock before the import.
quant_loss.py imports a `scenenet_pipeline` package that is not in the reference's tree: its two modules are pointed at the
reference's own core.criterions.w_mse / geneo_loss.  QuantileLoss.__init__ hands seven positional arguments to a
WeightedMSE.__init__ that takes six and raises, so the instance is made with __new__, initialised by the reference's
WeightedMSE.__init__ and given its `qs` by hand, as the constructor would have set them (quant_loss.py:57-58).  Its methods
then run unmodified.
"""
import importlib
import os
import sys
import tempfile
import warnings
from unittest.mock import MagicMock

import numpy as np
import torch

sys.dont_write_bytecode = True
REF = os.environ.get("SCENENET_REFERENCE")
if not REF or not os.path.isdir(REF):
    sys.exit("set SCENENET_REFERENCE to a checkout of the reference")
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))
sys.path.append(os.path.dirname(os.path.dirname(OUT)))   # the repository root: tests/quantile_cases.py imports `oracle`

for name in ["pyntcloud", "open3d", "laspy", "webcolors", "sympytorch", "IPython", "IPython.display", "seaborn",
             "torchvision", "torchvision.transforms", "pytorch_lightning", "pytorch_lightning.callbacks", "wandb",
             "torchmetrics", "torchviz", "torchsummary", "sklearn", "sklearn.metrics", "sklearn.cluster", "cloudpickle",
             "sympy", "tqdm", "matplotlib", "matplotlib.pyplot", "matplotlib.cm"]:
    try:
        importlib.import_module(name)
    except Exception:
        sys.modules[name] = MagicMock()

sys.path.insert(0, REF)
warnings.filterwarnings("ignore")

from core.criterions import geneo_loss as ref_geneo_loss  # noqa: E402
from core.criterions import w_mse as ref_w_mse  # noqa: E402

for name in ["scenenet_pipeline", "scenenet_pipeline.torch_geneo", "scenenet_pipeline.torch_geneo.criterions"]:
    sys.modules[name] = MagicMock()
sys.modules["scenenet_pipeline.torch_geneo.criterions.w_mse"] = ref_w_mse
sys.modules["scenenet_pipeline.torch_geneo.criterions.geneo_loss"] = ref_geneo_loss

from core.criterions.focal_loss import FocalLoss  # noqa: E402
from core.criterions.iou_loss import IoULoss  # noqa: E402
from core.criterions.quant_loss import QuantileLoss  # noqa: E402

import quantile_cases as qc  # noqa: E402


def reference_criterion(targets, qs, alpha, epsilon):
    crit = QuantileLoss.__new__(QuantileLoss)
    ref_w_mse.WeightedMSE.__init__(crit, targets, os.path.join(os.getcwd(), "no_such_file.pickle"), alpha, epsilon)
    crit.qs = qs.reshape(-1, 1).to(crit.device)
    crit._qs = torch.concat((crit.qs, crit.qs - 1), dim=-1).to(crit.device)
    return crit


def main():
    out = {}
    qs = torch.tensor(qc.GOLDEN_QS)
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)   # (the reference's WeightedMSE writes ./hist_estimation.pickle)
        try:
            for B in (1, 2):
                pred0, gt = qc.golden_inputs(B)
                crit = reference_criterion(gt, qs, qc.GOLDEN_HP["alpha"], qc.GOLDEN_HP["epsilon"])
                pred = pred0.clone().requires_grad_(True)
                loss = crit.forward(pred, gt)
                loss.backward()
                ties = int((pred0 == gt).sum())
                out[f"b{B}|pred"] = pred0.numpy()
                out[f"b{B}|gt"] = gt.numpy()
                out[f"b{B}|freqs"] = crit.freqs.numpy()
                out[f"b{B}|ranges"] = crit.ranges.numpy()
                out[f"b{B}|quantile_loss"] = crit.quantile_loss(pred0, gt).numpy()
                out[f"b{B}|weights"] = crit.get_weight_target(gt).numpy()
                out[f"b{B}|loss"] = loss.detach().numpy()
                out[f"b{B}|grad"] = pred.grad.numpy()
                print(f"B = {B}: loss {float(loss):.9g}  quantile_loss {tuple(out[f'b{B}|quantile_loss'].shape)}  "
                      f"ties {ties} of {pred0.numel()} (at zero: {int(((pred0 == gt) & (gt == 0)).sum())})")
        finally:
            os.chdir(cwd)
    p0, t = qc.golden_pair()
    out["pair|inputs"], out["pair|targets"] = p0.numpy(), t.numpy()
    for red in ("mean", "sum", "none"):
        p = p0.clone().requires_grad_(True)
        loss = FocalLoss(reduction=red, alpha=0.25, gamma=2)(p, t)
        loss.sum().backward()
        out[f"pair|focal_{red}|loss"] = loss.detach().numpy()
        out[f"pair|focal_{red}|grad"] = p.grad.numpy()
    out["pair|focal_alpha"], out["pair|focal_gamma"] = np.array(0.25), np.array(2.0)
    for smooth in (1, 0.5):
        p = p0.clone().requires_grad_(True)
        loss = IoULoss()(p, t, smooth=smooth)
        loss.backward()
        out[f"pair|iou_{smooth}|loss"] = loss.detach().numpy()
        out[f"pair|iou_{smooth}|grad"] = p.grad.numpy()
    out["qs"] = qs.numpy()
    out["hp"] = np.array([qc.GOLDEN_HP["alpha"], qc.GOLDEN_HP["epsilon"]])
    path = os.path.join(OUT, "quantile_loss.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
