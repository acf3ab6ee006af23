"""
Generates tests/golden/class_colors.npz by IMPORTING the reference (dlavado/scene-net) where it is checked out
(SCENENET_REFERENCE) and running its own color_pointcloud(pcd, classes, class_color=table) (utils/pcd_processing.py:525-574)
on the class vectors of tests/voxel_classes_cases.golden_cases().  The reference never travels: only the class vectors, their
tables, their names and the colours it returned are committed.  Run from the repo root:

    SCENENET_REFERENCE=<checkout of the reference> python tests/golden/make_golden_class_colors.py

Third-party modules the reference imports for plotting / IO only are replaced by MagicMock before the import (SURVEY.md
8c); `pcd` is a MagicMock too -- open3d is a pass-through container in this function, so the colours are numpy's alone.
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
sys.path.append(os.path.dirname(os.path.dirname(OUT)))   # the repository root: tests/binning_cases.py imports `oracle`

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

import voxel_classes_cases as kc  # noqa: E402


def main():
    out = {}
    names = []
    for name, classes, table in kc.golden_cases():
        colors = ref_eda.color_pointcloud(MagicMock(), classes.copy(), class_color=table.copy())
        colors = np.ascontiguousarray(colors, dtype=np.float64)
        assert colors.shape == (len(classes), 3)
        names.append(name)
        out[name + "_classes"] = classes
        out[name + "_table"] = table
        out[name + "_colors"] = colors
        mine = kc.colors_loop(classes, table)
        print(f"{name:14s} n {len(classes):4d} {str(classes.dtype):8s} classes {len(np.unique(classes)):3d} table "
              f"{table.shape}  restatement equal: {mine.tobytes() == colors.tobytes()}")
    out["names"] = np.array(names)
    path = os.path.join(OUT, "class_colors.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, {len(names)} cases")


if __name__ == "__main__":
    main()
