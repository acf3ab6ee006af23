"""
Generates tests/golden/avg_dist_points.npz by IMPORTING the reference (dlavado/scene-net) where it is checked out
(SCENENET_REFERENCE) and running its own avg_dist_points(xyz, accuracy, num_dists) (utils/pcd_processing.py:477-505) on the
clouds of tests/knn_cases.golden_clouds().  The reference never travels: only the clouds, the arguments, their names and
the floats it returned are committed.  Run from the repo root:

    SCENENET_REFERENCE=<checkout of the reference> python tests/golden/make_golden_avg_dist.py

Third-party modules the reference imports for plotting / IO only are replaced by MagicMock before the import (SURVEY.md
8c); avg_dist_points itself is numpy alone.
"""
import importlib
import os
import sys
import warnings
from unittest.mock import MagicMock

import numpy as np

sys.dont_write_bytecode = True
REF = os.environ.get("SCENENET_REFERENCE")
if not REF or not os.path.isdir(REF):
    sys.exit("set SCENENET_REFERENCE to a checkout of the reference")
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))
sys.path.append(os.path.dirname(os.path.dirname(OUT)))   # the repository root

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

from utils import pcd_processing as ref_eda  # noqa: E402

import knn_cases as kc  # noqa: E402


def main():
    out, names = {}, []
    for name, xyz, accuracy, num_dists in kc.golden_clouds():
        value = float(ref_eda.avg_dist_points(xyz.copy(), accuracy, num_dists))
        names.append(name)
        out[name + "_xyz"] = xyz
        out[name + "_args"] = np.array([accuracy, num_dists], dtype=np.float64)
        out[name + "_value"] = np.array(value, dtype=np.float64)
        mine = kc.avg_dist_points_host(xyz, accuracy, num_dists)
        m = round(len(xyz) * accuracy)
        rel = abs(mine - value) / abs(value)
        print(f"{name:12s} m {len(xyz):3d} view {m:3d} num_dists {num_dists:2d}  reference {value!r}  restatement {mine!r}  "
              f"rel {rel:.2e}  bound {kc.avg_dist_bound(m, num_dists):.2e}")
    out["names"] = np.array(names)
    path = os.path.join(OUT, "avg_dist_points.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, {len(names)} cases")


if __name__ == "__main__":
    main()
