"""
Generates tests/golden/voxel_cloud.npz by IMPORTING the reference (dlavado/scene-net) where it is checked out
(SCENENET_REFERENCE) and running its own plot_voxelgrid(grid, color_mode, plot=False) (utils/voxelization.py:45-144) on the
grids of tests/voxel_cloud_cases.golden_cases().  The reference never travels: only the grids, their names and the rows it
returned are committed ("None" as an empty (0, 0) array with `<name>_none` = 1).  Run from the repo root:

    SCENENET_REFERENCE=<checkout of the reference> python tests/golden/make_golden_voxel_cloud.py

Third-party modules the reference imports for plotting / IO only are replaced by MagicMock before the import (SURVEY.md
8c); open3d is a pass-through container in this function, so the rows are numpy's alone.  matplotlib must be the real one:
the `ranges` colours are cm.jet's.
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

import matplotlib.cm  # noqa: E402,F401  (never mocked)

for name in ["pyntcloud", "open3d", "laspy", "webcolors", "sympytorch", "IPython", "IPython.display", "seaborn",
             "torchvision", "torchvision.transforms", "pytorch_lightning", "pytorch_lightning.callbacks", "wandb",
             "torchmetrics", "torchviz", "torchsummary", "pandas", "sklearn", "sklearn.metrics", "sklearn.cluster"]:
    try:
        importlib.import_module(name)
    except Exception:
        sys.modules[name] = MagicMock()

sys.path.insert(0, REF)
warnings.filterwarnings("ignore")

from utils import voxelization as ref_vox  # noqa: E402

import voxel_cloud_cases as vc  # noqa: E402


def main():
    out = {}
    names, modes, rs = [], [], []
    for name, grid, mode, r in vc.golden_cases():
        rows = ref_vox.plot_voxelgrid(grid.copy(), color_mode=mode, plot=False, r=r)
        names.append(name)
        modes.append(mode)
        rs.append(r)
        out[name + "_grid"] = grid
        out[name + "_none"] = np.array([rows is None], dtype=np.uint8)
        if rows is None:
            rows = np.empty((0, 0))
        rows = np.ascontiguousarray(rows, dtype=np.float64)
        assert rows.ndim == 2
        out[name + "_rows"] = rows
        mine = vc.restate(grid, mode, r, vc.jet_table(r) if mode == "ranges" else None)
        same = (mine is None and rows.shape == (0, 0)) or (mine is not None and mine.shape == rows.shape
                                                           and mine.tobytes() == rows.tobytes())
        print(f"{name:22s} {str(grid.shape):12s} {grid.dtype} {mode:8s} r={r:2d} rows {rows.shape}  restatement equal: {same}")
    out["names"], out["modes"], out["rs"] = np.array(names), np.array(modes), np.array(rs, dtype=np.int64)
    for r in (2, 5, 10, 17):
        out[f"jet_{r}"] = vc.jet_table(r)
    path = os.path.join(OUT, "voxel_cloud.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, {len(names)} cases")


if __name__ == "__main__":
    main()
