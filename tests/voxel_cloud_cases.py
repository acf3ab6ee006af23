"""K16 voxel clouds: the numpy restatement of the reference's plot_voxelgrid(grid, color_mode, plot=False) rows
(utils/voxelization.py:45-144 with utils/pcd_processing.py:525-574 behind it), and the case sets the host and the GPU tests
share.  The restatement is pinned to the reference's own output by tests/golden/voxel_cloud.npz
(tests/golden/make_golden_voxel_cloud.py, byte for byte).  Two rules are BUILD-DEFINED -- the reference has no such form --
and pinned only here: the `desc` form (voxel centres, size-mode padding cells left out) and `rgb16`."""
import numpy as np

MODES = ("density", "ranges")


def lin_step(r):
    return np.linspace(0, 1, r), (1 / r) / 2


def jet_table(r):
    """cm.jet(np.linspace(0, 1, r))[:, :3] with row 0 forced to white; needs matplotlib"""
    import matplotlib.cm as cm
    t = np.array(cm.jet(np.linspace(0, 1, r)))[:, :3].astype(np.float64)
    t[0] = 1.0
    return np.ascontiguousarray(t)


def live_mask(grid, mode, r=10):
    v = np.asarray(grid).astype(np.float64)
    if mode == "density":
        return v != 0
    lin, _ = lin_step(r)
    with np.errstate(invalid="ignore"):
        return v > lin[1]


def colours(values, mode, r=10, table=None):
    """[N,3] fp64: 255 * the colour of every value (already widened to fp64), one rounding per operation"""
    c = np.asarray(values, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        if mode == "density":
            ch = np.where(c < 0, 1.0 + c, 1.0 - c)
            one = np.ones_like(c)
            rgb = np.where((c < 0)[:, None], np.stack([ch, ch, one], axis=1), np.stack([one, ch, ch], axis=1))
            return rgb * 255.0
        lin, step = lin_step(r)
        if len(c) == 0:
            return np.empty((0, 3))
        idx = np.argmin(np.abs(c[:, None] - lin - step), axis=-1)
        return np.asarray(table, dtype=np.float64)[idx] * 255.0


def restate(grid, mode, r=10, table=None):
    """What the reference returns for one [Z, X, Y] grid: None, a (0, 6) array or the (N, 6) fp64 rows.  A NaN voxel in the
    density mode (the reference raises IndexError) gives the row (x, y, z, 255, NaN, NaN): the build's rule."""
    v = np.asarray(grid).astype(np.float64)
    z, x, y = (v != 0).nonzero()
    if len(z) == 0:
        return None
    vals = v[z, x, y]
    if mode == "ranges":
        keep = live_mask(vals, "ranges", r)
        z, x, y, vals = z[keep], x[keep], y[keep], vals[keep]
    xyz = np.stack([x, y, z], axis=1).astype(np.float64)
    return np.concatenate([xyz, colours(vals, mode, r, table)], axis=1)


def bad_counts(grid, mode, keep=None):
    """(NaN cells kept, kept cells that are not NaN whose colour leaves [0, 255]) -- density only, (0, 0) otherwise"""
    if mode != "density":
        return 0, 0
    v = np.asarray(grid).astype(np.float64)
    live = v != 0
    if keep is not None:
        live &= keep
    vals = v[live]
    nan = np.isnan(vals)
    with np.errstate(invalid="ignore"):
        ch = np.where(vals < 0, 1.0 + vals, 1.0 - vals) * 255.0
        out = ~nan & ((ch < 0) | (ch > 255))
    return int(nan.sum()), int(out.sum())


def rgb16(rows_rgb):
    """build-defined: clamp(rint(255 c), 0, 255) * 257, NaN -> 0"""
    t = np.asarray(rows_rgb, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        q = np.clip(np.rint(t), 0, 255)
    q = np.where(np.isnan(t), 0.0, q)
    return (q.astype(np.int64) * 257).astype(np.uint16)


def desc_keep(desc_row, nz, nx, ny):
    """[nz, nx, ny] bool: cells whose upper edge on every axis is finite (a size-mode padding cell is not part of the tile)"""
    ex, ey, ez = desc_edges(desc_row, nz, nx, ny)
    fx, fy, fz = np.isfinite(ex[1:]), np.isfinite(ey[1:]), np.isfinite(ez[1:])
    return fz[:, None, None] & fx[None, :, None] & fy[None, None, :]


def desc_edges(desc_row, nz, nx, ny):
    d = np.asarray(desc_row, dtype=np.float64)
    ex = d[6:6 + nx + 1]
    ey = d[6 + nx + 1:6 + nx + ny + 2]
    ez = d[6 + nx + ny + 2:6 + nx + ny + nz + 3]
    return ex, ey, ez


def restate_desc(grid, desc_row, mode, r=10, table=None):
    """build-defined: the rows of `restate` with x, y, z the voxel centres (e[k] + e[k+1]) * 0.5 and the padding cells left
    out; always an (N, 6) array"""
    v = np.asarray(grid).astype(np.float64)
    nz, nx, ny = v.shape
    live = live_mask(v, mode, r) & desc_keep(desc_row, nz, nx, ny)
    z, x, y = live.nonzero()
    ex, ey, ez = desc_edges(desc_row, nz, nx, ny)
    with np.errstate(invalid="ignore"):
        xyz = np.stack([(ex[x] + ex[x + 1]) * 0.5, (ey[y] + ey[y + 1]) * 0.5, (ez[z] + ez[z + 1]) * 0.5], axis=1)
    return np.concatenate([xyz.reshape(-1, 3), colours(v[z, x, y], mode, r, table)], axis=1)


# --------------------------------------------------------------------------- #
def seam_values(r):
    """the values on every seam of the ranges rule at r, and of the density rule: the filter edge lin[1] and its
    successor, every bin boundary (where the argmin changes rows) and its two neighbours, 1.0, negatives, values above 1"""
    lin, step = lin_step(r)
    vals = [lin[1], np.nextafter(lin[1], 2.0), np.nextafter(lin[1], -1.0), 1.0, np.nextafter(1.0, 2.0), np.nextafter(1.0, 0.0),
            -1.0, -0.25, -1e-300, 1e-300, 1.5, 2.0, -1.5, 0.5]
    for j in range(r):
        for b in (lin[j], lin[j] + step, (lin[j] + lin[min(j + 1, r - 1)]) / 2 + step, (lin[j] + lin[min(j + 1, r - 1)]) / 2):
            vals += [b, np.nextafter(b, 2.0), np.nextafter(b, -1.0)]
    return np.array(vals, dtype=np.float64)


def seam_grid(shape, r, dtype, seed):
    """a grid of `shape` ([Z, X, Y]) about half zero, with random values in [-1.2, 1.6] and the seam values of r planted
    (rounded to `dtype`, and in f32 the neighbours of the ROUNDED seams as well); one -0.0"""
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    v = rng.uniform(-1.2, 1.6, n)
    v[rng.random(n) < 0.5] = 0.0
    seams = seam_values(r).astype(dtype)
    if dtype == np.float32:
        seams = np.concatenate([seams, np.nextafter(seams, np.float32(2)), np.nextafter(seams, np.float32(-2))])
    seams = seams[:n - 1]
    pos = rng.permutation(n)[:len(seams) + 1]
    v = v.astype(dtype)
    v[pos[:-1]] = seams
    v[pos[-1]] = -0.0
    return v.reshape(shape)


GOLDEN_SHAPES = ((9, 8, 7), (5, 8, 7), (9, 4, 7), (7, 8, 3))


def golden_cases():
    """name, grid, mode, r of every case of tests/golden/voxel_cloud.npz (the generator and the tests build them alike)"""
    cases = []
    k = 0
    for dtype, tag in ((np.float32, "f32"), (np.float64, "f64")):
        for r in (2, 5, 10, 17):
            shape = GOLDEN_SHAPES[k % len(GOLDEN_SHAPES)]
            g = seam_grid(shape, r, dtype, seed=100 + k)
            cases.append((f"ranges_r{r}_{tag}", g, "ranges", r))
            if r in (5, 10):
                cases.append((f"density_r{r}_{tag}", g, "density", r))
            k += 1
        cases.append((f"zero_{tag}", np.zeros((3, 4, 5), dtype=dtype), "density", 10))
        cases.append((f"zero_ranges_{tag}", np.zeros((3, 4, 5), dtype=dtype), "ranges", 10))
        low = np.zeros((4, 3, 5), dtype=dtype)
        edge = dtype(np.linspace(0, 1, 10)[1])     # the filter edge itself is dropped; in f32, the nearest value not above it
        if np.float64(edge) > np.linspace(0, 1, 10)[1]:
            edge = np.nextafter(edge, dtype(0))
        low.reshape(-1)[::3] = np.array([0.05, -0.5, 0.1, edge], dtype=dtype)[np.arange(20) % 4]
        cases.append((f"filtered_{tag}", low, "ranges", 10))
    return cases


# --------------------------------------------------------------------------- #
def torch_dtype_grids(shape, seed):
    """name -> [Z, X, Y] numpy grid for every dtype the kernel takes (bool as numpy bool)"""
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    out = {"f32": seam_grid(shape, 10, np.float32, seed), "f64": seam_grid(shape, 10, np.float64, seed + 1)}
    u8 = rng.integers(0, 4, n).astype(np.uint8)
    u8[rng.random(n) < 0.4] = 0
    u8[:3] = (255, 1, 0)
    out["u8"] = u8.reshape(shape)
    out["bool"] = (rng.random(n) < 0.3).reshape(shape)
    return out
