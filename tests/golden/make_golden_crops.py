"""
Generates tests/golden/scan_crops.npz by IMPORTING the reference (dlavado/scene-net) where it is checked out
(SCENENET_REFERENCE) and running its own crops on the rows of ts40k_sample575_full.npz.  The reference never travels:
only the centres, radii and one membership bit per point and crop are committed.  Run from the repo root:

    SCENENET_REFERENCE=<checkout of the reference> python tests/golden/make_golden_crops.py

Third-party modules the reference imports for plotting / IO only are replaced by MagicMock before the import (SURVEY.md
8c); utils/pcd_processing.py's crop functions are numpy only and run unmodified.
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

for name in ["pyntcloud", "open3d", "laspy", "webcolors", "sympytorch", "IPython", "IPython.display", "seaborn",
             "torchvision", "torchvision.transforms", "pytorch_lightning", "pytorch_lightning.callbacks", "wandb",
             "torchmetrics", "torchviz", "torchsummary"]:
    try:
        importlib.import_module(name)
    except Exception:
        sys.modules[name] = MagicMock()

sys.path.insert(0, REF)
warnings.filterwarnings("ignore")

from utils import pcd_processing as eda  # noqa: E402


def membership(scan, rows):
    """One bit per scan row: the returned rows are scan[mask] in scan order, and the tile has no duplicate rows among
    members and non-members alike -- checked, so the bits ARE the reference's mask."""
    keys = {r.tobytes(): i for i, r in enumerate(scan)}
    assert len(keys) == len(scan), "the tile has duplicate rows: membership cannot be read off the returned rows"
    idx = np.array([keys[r.tobytes()] for r in np.ascontiguousarray(rows)], dtype=np.int64)
    assert np.all(np.diff(idx) > 0), "rows come back in scan order"
    mask = np.zeros(len(scan), dtype=bool)
    mask[idx] = True
    assert np.array_equal(scan[mask], rows)
    return np.packbits(mask)


def main():
    tile = np.load(os.path.join(OUT, "ts40k_sample575_full.npz"))["tile"]
    xyz, classes = np.ascontiguousarray(tile[:, :3]), np.ascontiguousarray(tile[:, 3])
    scan = np.ascontiguousarray(tile[:, :4])
    out = {}
    rng = np.random.default_rng(0)
    lo, hi = xyz.min(axis=0), xyz.max(axis=0)
    centres = lo + rng.random((6, 3)) * (hi - lo)
    radii = np.array([0.0, 3.0, 7.5])
    out["at_centres"], out["at_radii"] = centres, radii
    used = []
    for j, r in enumerate(radii):
        used.append(np.max(xyz[:, 2]) - np.min(xyz[:, 2]) if r == 0 else r)
        samples = eda.crop_at_locations(xyz, centres, radius=r, classes=classes)
        for i, s in enumerate(samples):
            assert s.shape[1] == 4
            out[f"at_{j}_{i}_bits"] = membership(scan, s)
    out["at_radii_used"] = np.array(used)

    tower = xyz[classes == 15]
    assert len(tower) > 1
    out["tower_index"] = np.flatnonzero(classes == 15).astype(np.int64)
    out["tower_baricentre"] = np.mean(tower, axis=0)
    t_radii = np.array([0.0, 5.0, 15.0])
    out["tower_radii"] = t_radii
    used = []
    for j, r in enumerate(t_radii):
        used.append(np.max(tower[:, 2]) - np.min(tower[:, 2]) if r == 0 else r)
        rad, c = eda.crop_tower_radius(xyz, classes, tower, radius=r)
        assert c.dtype.kind == "i" and rad.shape[1] == 3
        out[f"tower_{j}_bits"] = membership(scan, np.column_stack([rad, c.astype(np.float64)]))
    out["tower_radii_used"] = np.array(used)

    half = len(tower) // 2
    a, c = eda.crop_two_towers(xyz, classes, tower[:half], tower[half:])
    out["two_bits"] = membership(scan, np.column_stack([a, c.astype(np.float64)]))
    out["two_split"] = np.array([half], dtype=np.int64)
    out["two_min"], out["two_max"] = tower.min(axis=0), tower.max(axis=0)

    path = os.path.join(OUT, "scan_crops.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, {sum(k.endswith('_bits') for k in out)} crops")


if __name__ == "__main__":
    main()
