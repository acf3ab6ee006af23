"""What the foreign-point binning tests share (tests/test_binning_host.py, tests/test_gpu_binning_foreign.py): the binning
rule of K1 written once in numpy fp64, applied to points a grid was NOT built from, the generator of such points, the
descriptors the tests bin them with (built on the host with the oracle's arithmetic, so the GPU file can compare the
device's tables with them bit for bit) and the expected outputs of the scatter, the bitmap and the read-back kernels.
No test lives here."""
import numpy as np

from oracle import voxel_oracle as vo

# (x, y, z) grids of the n-mode descriptors, and why each is there
DIMS = [(5, 7, 3),       # V % 32 != 0: no LDS bitmap, voxelize_batch must take the counting kernels
        (8, 12, 4),      # ny no multiple of 32: the row-emptiness proof straddles words
        (16, 32, 8),     # ny = 32: the proof rides on the merged words
        (64, 64, 64)]    # the production grid
SLAB_DIMS = (64, 128, 128)   # two z-slabs of the bitmap, four with the tower plane: `dropped` is counted once
CAPACITY = (32, 32, 32)      # size mode: the table every tile's own (n_x, n_y, n_z) is padded to
VOXEL_SIZE = (1.7, 1.9, 1.6)
KEEP = [15.0, 16.0]
LABELS = np.array([15.0, 16.0, 2.0, 7.0])
UTM = np.array([5.44e5 + 0.37, 4.634e6 - 0.11, 149.93])


def desc_len(dims):
    return 6 + sum(dims) + 3


def tables_of(desc_row, dims, own_dims=None):
    """The three edge tables of a descriptor row (lo[3], hi[3], edges x, y, z of the table's dims); with `own_dims` (size
    mode) only the tile's own n_a + 1 edges of each axis."""
    nx, ny, nz = dims
    own = dims if own_dims is None else tuple(int(v) for v in own_dims)
    d = np.asarray(desc_row, dtype=np.float64)
    start = (6, 6 + nx + 1, 6 + nx + ny + 2)
    return [d[s:s + n + 1] for s, n in zip(start, own)], own


def axis_index(edges, p):
    """THE RULE (oracle/voxel_oracle.py:73 for arbitrary p): largest j with e[j] < p, clipped to [0, n].  n means outside
    the table; numpy sorts NaN last, so NaN is outside; anything at or below e[0], -inf included, is bin 0."""
    n = len(edges) - 1
    return np.clip(np.searchsorted(edges, p, side="left") - 1, 0, n)


def expected_flat(desc_row, dims, pts, own_dims=None):
    """(iz * nx + ix) * ny + iy in the table's dims, -1 for a point outside the table on any axis."""
    nx, ny, nz = dims
    (ex, ey, ez), own = tables_of(desc_row, dims, own_dims)
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    ix, iy, iz = axis_index(ex, pts[:, 0]), axis_index(ey, pts[:, 1]), axis_index(ez, pts[:, 2])
    out = (ix >= own[0]) | (iy >= own[1]) | (iz >= own[2])
    return np.where(out, -1, (iz * nx + ix) * ny + iy).astype(np.int64)


def shares(desc_row, dims, pts, own_dims=None):
    """(outside, clipped low on some axis without being outside, plainly inside) as fractions, and the rows with a NaN."""
    (ex, ey, ez), _ = tables_of(desc_row, dims, own_dims)
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    out = expected_flat(desc_row, dims, pts, own_dims) < 0
    low = ((pts[:, 0] <= ex[0]) | (pts[:, 1] <= ey[0]) | (pts[:, 2] <= ez[0])) & ~out
    n = float(len(pts))
    return out.sum() / n, low.sum() / n, (~out & ~low).sum() / n, int(np.isnan(pts).any(axis=1).sum())


# ---------------------------------------------------------------- points a grid was not built from
def foreign_points(lo, hi, dims, rng, n_random):
    """Per axis: every edge of the table, each edge +- one ulp, lo - span, hi + span, +-1e300, +-inf and NaN, the other two
    coordinates uniform inside the box; n_random points uniform over the box enlarged by 25 % on every side; three
    all-NaN rows.  Shuffled."""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    span = hi - lo
    rows = []
    for a in range(3):
        e = vo.linspace_edges(lo[a], hi[a], int(dims[a]))
        vals = np.concatenate([e, np.nextafter(e, np.inf), np.nextafter(e, -np.inf),
                               [lo[a] - span[a], hi[a] + span[a], 1e300, -1e300, np.inf, -np.inf, np.nan]])
        p = lo + rng.random((len(vals), 3)) * span
        p[:, a] = vals
        rows.append(p)
    rows.append((lo - 0.25 * span) + rng.random((int(n_random), 3)) * (1.5 * span))
    rows.append(np.full((3, 3), np.nan))
    pts = np.concatenate(rows)
    rng.shuffle(pts, axis=0)
    return pts


def own_cloud(b, n=400):
    """An in-box cloud at UTM scale whose extents (hence its cube, and its size-mode dims) differ per tile."""
    rng = np.random.default_rng(900 + b)
    ext = np.array([24.0, 18.0, 9.0]) * (1.0 + 0.2 * b)
    return UTM + 13.0 * b + rng.random((n, 3)) * ext


def bounds_box(b):
    """A non-cubic caller-given box at UTM scale, another one per tile."""
    lo = UTM + np.array([50.0, -20.0, 3.0]) * b
    return np.concatenate([lo, lo + np.array([97.3, 61.9, 23.7]) * (1.0 + 0.2 * b)])


def host_desc(kind, dims, B):
    """The descriptors of B tiles with numpy's arithmetic: kind "own" (the cube of own_cloud(b): what sn_voxel_prepare
    gives), "bounds" (bounds_box(b) as given: sn_voxel_desc_from_bounds) or "sized" (size mode on own_cloud(b) with
    VOXEL_SIZE, padded with +inf to `dims`: sn_voxel_desc_sized).  Returns (desc [B, desc_len], own dims [B, 3] | None)."""
    desc = np.empty((B, desc_len(dims)))
    own = np.empty((B, 3), dtype=np.int64) if kind == "sized" else None
    for b in range(B):
        if kind == "bounds":
            bb = bounds_box(b)
            lo, hi, n = bb[:3], bb[3:], dims
        else:
            g = vo.voxelgrid_compute(own_cloud(b), n_xyz=dims if kind == "own" else None,
                                     sizes=VOXEL_SIZE if kind == "sized" else None)
            lo, hi, n = g["xyzmin"], g["xyzmax"], tuple(int(v) for v in g["x_y_z"])
        if own is not None:
            own[b] = n
        edges = []
        for a in range(3):
            e = np.full(dims[a] + 1, np.inf)
            e[:n[a] + 1] = vo.linspace_edges(lo[a], hi[a], n[a])
            edges.append(e)
        desc[b] = np.concatenate([lo, hi] + edges)
    return desc, own


def n_random_for(dims):
    """Random points per full foreign set: enough that the out / low / inside shares of tests/test_binning_host.py hold
    next to the 3 (n_x + n_y + n_z + 3) + 21 edge points, and a tile stays within 1-5 k points."""
    return 4000 if sum(dims) > 100 else 1500


def foreign_batch(desc, dims, own=None, seed=0):
    """The batch of the GPU tests for descriptors desc [>= 3 rows]: tiles of 1001, 1 and 2 + n points (an odd start offset;
    a one-point tile whose point is outside), each tile's points made for ITS table.  Returns (tiles, labels)."""
    rng = np.random.default_rng(1234 + seed)
    tiles = []
    for b in (0, 2):
        d = own[b] if own is not None else dims
        tiles.append(foreign_points(desc[b, :3], desc[b, 3:6], d, rng, n_random_for(d)))
    first, last = tiles[0][:1001], np.concatenate([tiles[1], tiles[1][:2]])
    assert len(first) == 1001
    lo1, hi1 = desc[1, :3], desc[1, 3:6]
    one = (lo1 + 0.5 * (hi1 - lo1))[None].copy()
    one[0, 1] = hi1[1] + 0.5 * (hi1[1] - lo1[1])          # beyond the last y edge
    tiles = [first, one, last]
    labels = [LABELS[rng.integers(0, len(LABELS), len(t))] for t in tiles]
    return tiles, labels


# ---------------------------------------------------------------- expected outputs
def expected_scatter(desc, dims, tiles, labels=None, keep=KEEP, own=None):
    """counts, towers [B, nz, nx, ny] i64 and dropped [B] by np.bincount of expected_flat."""
    nx, ny, nz = dims
    V = nx * ny * nz
    B = len(tiles)
    counts = np.zeros((B, nz, nx, ny), dtype=np.int64)
    towers = np.zeros((B, nz, nx, ny), dtype=np.int64)
    dropped = np.zeros(B, dtype=np.int64)
    for b, t in enumerate(tiles):
        f = expected_flat(desc[b], dims, t, None if own is None else own[b])
        ins = f >= 0
        counts[b] = np.bincount(f[ins], minlength=V).reshape(nz, nx, ny)
        if labels is not None:
            k = ins & np.isin(labels[b], np.asarray(keep))
            towers[b] = np.bincount(f[k], minlength=V).reshape(nz, nx, ny)
        dropped[b] = (~ins).sum()
    return counts, towers, dropped


def expected_occ(counts):
    """ToFullDense(normalize_xyz(counts)) per tile: what the bitmap kernels (and their exact fallback) must give."""
    return np.stack([vo.to_full_dense(vo.normalize_xyz(c.astype(np.float64))) for c in counts])


def expected_gather(grid, desc, dims, tiles, fill, own=None):
    """grid [B, C, nz, nx, ny] -> [C, total]: tile b's points read tile b's grid, points outside get `fill`.  A tile may be
    empty ([0, 3])."""
    B, C = grid.shape[:2]
    g = grid.reshape(B, C, -1)
    cols = []
    for b, t in enumerate(tiles):
        f = expected_flat(desc[b], dims, t, None if own is None else own[b])
        v = g[b][:, np.maximum(f, 0)]
        v[:, f < 0] = fill
        cols.append(v)
    return np.concatenate(cols, axis=1)
