"""
Generates tests/golden/scan_census.npz by IMPORTING the reference (dlavado/scene-net) where it is checked out
(SCENENET_REFERENCE) and running its own crop_ground_samples (utils/pcd_processing.py:742-762) on a synthetic labelled
scan.  The reference never travels: only the scan and, per accepted sample, one membership bit per scan row and the class
column it returned are committed.  Run from the repo root:

    SCENENET_REFERENCE=<checkout of the reference> python tests/golden/make_golden_census.py

Third-party modules the reference imports for plotting / IO only are replaced by MagicMock before the import (SURVEY.md
8c); crop_ground_samples is numpy only and runs unmodified.

The scan: x extent exactly 960 m, so step = int(960 / 100) = 9: nine slabs of 9 m that start every 120 m.  Coordinates
sit on a 2^-10 m lattice at a UTM-like origin and the points are concentrated in and around the slabs, which keeps the
file small.  Among the slabs that hold points there is one for each cause of rejection -- a tower point (15.7, which
astype(int) makes 15), a single class, exactly 300 points, and the last slab, which holds the xmax point alone -- and
four that are accepted, one of them with exactly 301 points, one with classes that are not integers (2.9, 14.99, 16.0,
-0.5: none truncates to 15), one with a point exactly on x0 + 9 and one an ulp beyond it.
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

ORIGIN = np.array([5.44e5, 4.634e6, 1.5e2])
EXTENT, STEP = 960.0, 9
# (slab, points, classes drawn from, what becomes of it)
SLABS = ((0, 301, (0.0, 2.0), "accepted: one more than 300"),
         (1, 420, (2.9, 14.99, 16.0, -0.5), "accepted: classes that are not integers"),
         (2, 650, (0.0, 2.0, 5.0), "accepted"),
         (3, 500, (0.0, 2.0), "rejected: a tower point"),
         (4, 350, (1.0, 3.0), "accepted: a point on x0 + 9, another an ulp beyond"),
         (5, 380, (2.0,), "rejected: a single class"),
         (6, 300, (0.0, 2.0), "rejected: exactly 300 points"),
         (8, 1, (2.0,), "rejected: the xmax point alone"))


def membership(scan, rows):
    """One bit per scan row: the returned rows are scan[mask] in scan order (x, y, z as they are, the class column
    through astype(int)), and no two scan rows share their coordinates -- checked, so the bits ARE the reference's mask."""
    keys = {r.tobytes(): i for i, r in enumerate(np.ascontiguousarray(scan[:, :3]))}
    assert len(keys) == len(scan), "the scan has duplicate points: membership cannot be read off the returned rows"
    idx = np.array([keys[r.tobytes()] for r in np.ascontiguousarray(rows[:, :3])], dtype=np.int64)
    assert np.all(np.diff(idx) > 0), "rows come back in scan order"
    mask = np.zeros(len(scan), dtype=bool)
    mask[idx] = True
    assert np.array_equal(scan[mask, :3], rows[:, :3])
    assert np.array_equal(rows[:, 3], scan[mask, 3].astype(int).astype(np.float64))
    return np.packbits(mask)


def lattice(rng, lo, hi, size):
    return np.round(rng.uniform(lo, hi, size) * 1024.0) / 1024.0


def make_scan():
    rng = np.random.default_rng(12)
    xmin = ORIGIN[0]
    starts = np.linspace(xmin, xmin + EXTENT, STEP)
    rows = []
    for slab, count, classes, _ in SLABS:
        x0 = starts[slab]
        if slab == 8:
            rows.append([xmin + EXTENT, ORIGIN[1] + 3.25, ORIGIN[2] + 1.0, classes[0]])
            continue
        x = lattice(rng, x0 + 0.01, x0 + STEP - 0.01, count)
        if slab == 0:
            x[0] = xmin                                       # the scan's xmin, on the slab's lower bound
        if slab == 4:
            x[0] = x0 + STEP                                  # on the upper bound: a member
        p = np.column_stack([x, ORIGIN[1] + lattice(rng, 0, 40, count), ORIGIN[2] + lattice(rng, 0, 30, count),
                             rng.choice(np.array(classes), count)])
        p[:len(classes), 3] = classes                         # every class is there
        if slab == 3:
            p[7, 3] = 15.7
        rows.append(p)
        if slab == 4:                                         # an ulp beyond the upper bound: not a member
            rows.append([np.nextafter(x0 + STEP, np.inf), ORIGIN[1] + 1.5, ORIGIN[2] + 2.0, 15.0])
        # around the slab: towers and other classes that must not count
        around = [lattice(rng, x0 + STEP + 0.5, x0 + STEP + 30, 25)]
        if slab:
            around.append(lattice(rng, x0 - 30, x0 - 0.5, 25))
        ax = np.concatenate(around)
        rows.append(np.column_stack([ax, ORIGIN[1] + lattice(rng, 0, 40, len(ax)), ORIGIN[2] + lattice(rng, 0, 30, len(ax)),
                                     rng.choice(np.array([15.0, 7.0]), len(ax))]))
    scan = np.vstack([np.atleast_2d(r) for r in rows])
    scan = np.ascontiguousarray(scan[rng.permutation(len(scan))])
    assert scan[:, 0].min() == xmin and scan[:, 0].max() == xmin + EXTENT
    return scan


def main():
    scan = make_scan()
    assert len(scan) <= 8000
    xyz, classes = np.ascontiguousarray(scan[:, :3]), np.ascontiguousarray(scan[:, 3])
    samples = eda.crop_ground_samples(xyz, classes)
    out = {"scan": scan, "n_samples": np.array([len(samples)], dtype=np.int64)}
    for i, s in enumerate(samples):
        assert s.shape[1] == 4 and s.dtype == np.float64
        out[f"sample_{i}_bits"] = membership(scan, s)
        out[f"sample_{i}_class"] = s[:, 3].astype(np.int16)
        assert np.array_equal(out[f"sample_{i}_class"].astype(np.float64), s[:, 3])
    sizes = [len(s) for s in samples]
    assert sizes == [301, 420, 650, 350], sizes
    path = os.path.join(OUT, "scan_census.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, {len(scan)} rows, samples of {sizes}")


if __name__ == "__main__":
    main()
