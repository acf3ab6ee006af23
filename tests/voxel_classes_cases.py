"""What the K18 tests share (tests/test_voxel_classes_host.py, tests/test_gpu_voxel_classes.py): the reference's
classes_on_voxel (utils/voxelization.py:232-239) restated literally in pandas over the project's own binning oracle
(tests/binning_cases.py::expected_flat -- pyntcloud is not installed, so its binning is not pinned here, as for K1 and K17),
a second formulation of the same grid in plain numpy, the reference's colour loop (utils/pcd_processing.py:555-564)
restated, the numpy restatement of the device's key map and the case builders.  No test lives here."""
import os
import warnings

import numpy as np
import pandas as pd

import binning_cases as bc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "class_colors.npz")
NAN_BITS = 0x7ff8000000000000
SPECIAL_LABELS = np.array([np.nan, np.inf, -np.inf, -3.0, -0.5, 1e300, -1e300, 5e-324, 15.0, 16.0, 2.0, 7.0])


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


# ---------------------------------------------------------------- the class grid
def grid_pandas(flat, labels, dims):
    """The reference's lines: the DataFrame, groupby(["z", "x", "y"]).max() and the loop into np.zeros; voxel_z / _x / _y
    are the binning oracle's, and a row the table does not hold (flat < 0) takes no part."""
    nx, ny, nz = dims
    flat = np.asarray(flat, dtype=np.int64)
    ins = flat >= 0
    f = flat[ins]
    voxel_z, rest = f // (nx * ny), f % (nx * ny)
    voxel_x, voxel_y = rest // ny, rest % ny
    data = np.zeros((nz, nx, ny))
    voxs = pd.DataFrame({"label": np.asarray(labels, dtype=np.float64)[ins],
                         "z": voxel_z, "x": voxel_x, "y": voxel_y})
    groups = voxs.groupby(["z", "x", "y"]).max()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", FutureWarning)       # the reference's own line: a one-element Series into a cell
        for i, hist in groups.iterrows():
            data[i] = hist
    return data


def grid_fmax(flat, labels, dims):
    """The same grid without pandas: np.fmax.at over the binned rows from NaN (fmax skips NaN), zero where nothing fell,
    NaN where only NaN labels fell."""
    nx, ny, nz = dims
    V = nx * ny * nz
    flat = np.asarray(flat, dtype=np.int64)
    labels = np.asarray(labels, dtype=np.float64)
    ins = flat >= 0
    f, lab = flat[ins], labels[ins]
    top = np.full(V, np.nan)
    np.fmax.at(top, f, lab)                                   # fmax(NaN, x) = x: NaN stays only where every label is NaN
    hit = np.bincount(f, minlength=V) > 0
    out = np.where(hit, top, 0.0)
    return out.reshape(nz, nx, ny)


def expected_grid(desc, dims, tiles, labels):
    """The whole batch by the reference's pandas lines: (grid [B,nz,nx,ny], unbinned [B], nan_labels [B]).  A size-mode
    descriptor is binned as it stands (own_dims None): the padding cells are cells."""
    grids, unb, nans = [], [], []
    for b, (t, lab) in enumerate(zip(tiles, labels)):
        flat = bc.expected_flat(desc[b], dims, t)
        grids.append(grid_pandas(flat, lab, dims))
        unb.append(int((flat < 0).sum()))
        nans.append(int(np.isnan(lab).sum()))
    return np.stack(grids), np.array(unb, dtype=np.int64), np.array(nans, dtype=np.int64)


def key_of(x):
    """The device's order-preserving key of an fp64 that is not NaN: the sign bit flipped for a value whose sign bit is
    clear, every bit inverted for one whose sign bit is set."""
    u = np.ascontiguousarray(np.asarray(x, dtype=np.float64)).view(np.uint64)
    neg = (u >> np.uint64(63)).astype(bool)
    return np.where(neg, ~u, u | np.uint64(1 << 63))


def special_labels(n, rng, nan_share=0.15):
    """n labels: SPECIAL_LABELS (NaN among them) drawn at random, more NaN mixed in"""
    lab = SPECIAL_LABELS[rng.integers(0, len(SPECIAL_LABELS), n)].copy()
    lab[rng.random(n) < nan_share] = np.nan
    return lab


def cube_tile(n, seed, extent=20.0):
    rng = np.random.default_rng(seed)
    return bc.UTM + rng.random((n, 3)) * extent


def own_desc(pts, dims):
    """The n-mode descriptor sn_voxel_prepare(regular=1) builds for one tile, with the oracle's arithmetic."""
    from oracle import voxel_oracle as vo
    g = vo.voxelgrid_compute(pts, n_xyz=dims)
    return np.concatenate([g["xyzmin"], g["xyzmax"]] + [vo.linspace_edges(g["xyzmin"][a], g["xyzmax"][a], dims[a])
                                                        for a in range(3)])


# ---------------------------------------------------------------- class colours
def colors_loop(classes, class_color):
    """The reference's loop, literally (IndexError where it raises)."""
    unique_classes = np.unique(classes)
    np_colors = np.empty((len(classes), 3))
    for i, c in enumerate(classes):
        np_colors[i, :] = class_color[np.where(unique_classes == c)[0][0]]
    return np_colors


def is_valid(classes):
    c = np.asarray(classes, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return (c >= 0) & (c <= 65535) & (np.floor(c) == c)


def expected_colors(classes, class_color):
    """What the device gives for one tile: (colors [n,3] with NaN rows where the reference raises, unique, bad, short)."""
    c = np.asarray(classes, dtype=np.float64)
    table = np.asarray(class_color, dtype=np.float64)
    ok = is_valid(c)
    unique = np.unique(c[ok])
    rank = np.searchsorted(unique, np.where(ok, c, 0.0))
    short = ok & (rank >= len(table))
    out = np.full((len(c), 3), np.nan)
    good = ok & ~short
    out[good] = table[rank[good]]
    return out, unique, int((~ok).sum()), int(short.sum())


def rgb16(colors):
    """clamp(rint(255 c), 0, 255) * 257, NaN -> 0: voxel_cloud's rule from the colour in 0 .. 1"""
    t = 255.0 * np.asarray(colors, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        q = np.clip(np.rint(t), 0, 255)
    q = np.where(np.isnan(t), 0.0, q)
    return (q.astype(np.int64) * 257).astype(np.uint16)


LAS_CLASSES = np.array([0, 1, 2, 3, 4, 5, 6, 7, 9, 15, 16, 17, 18, 31, 64, 255], dtype=np.float64)
KITTI_IDS = np.array([0, 1, 10, 11, 13, 15, 16, 18, 20, 30, 31, 32, 40, 44, 48, 49, 50, 51, 52, 60, 70, 71, 72, 80, 81, 99,
                      252, 253, 254, 255, 256, 257, 258, 259, 65535], dtype=np.float64)


def golden_cases():
    """[(name, classes [n], class_color [T,3])] the golden file holds, the reference's outputs aside."""
    rng = np.random.default_rng(1818)
    table = lambda t: rng.integers(0, 256, (t, 3)) / 255   # noqa: E731
    cases = []
    c = LAS_CLASSES[rng.integers(0, len(LAS_CLASSES), 400)]
    cases.append(("las", c, table(len(np.unique(c)))))
    c = KITTI_IDS[rng.integers(0, len(KITTI_IDS), 500)]
    cases.append(("kitti16", c, table(len(np.unique(c)) + 3)))                 # a table longer than it need be
    cases.append(("single", np.full(300, 15.0), table(1)))
    c = np.concatenate([np.arange(22.0), rng.integers(0, 22, 378).astype(np.float64)])
    rng.shuffle(c)
    cases.append(("all22", c, table(22)))
    c = rng.integers(0, 20, 350)                                              # an integer dtype, as laspy hands classes over
    cases.append(("int_dtype", c, table(22)))
    c = np.array([7.0, 2.0] * 100 + [65535.0, 0.0])
    cases.append(("two_and_ends", c, table(4)))
    return cases
