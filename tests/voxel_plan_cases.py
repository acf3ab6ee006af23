"""What the plan tests of K1's LDS-bitmap path share (tests/test_voxel_plan_host.py, tests/test_gpu_voxel_plans.py): the
table of grids with the fork each one selects and the eight words sn_voxel_occupancy_plan must report for it -- written
out by hand from the rules in csrc/voxel.hip (occ_slabs, SN_OCC_FUSED_PROOF, SN_OCC_VEC4, occ_finalize_blocks,
occ_binning_lds), never computed by the library --, a builder of point clouds from a prescribed integer count grid, and
the tile recipes that make the emptiness proof of occ_finalize_kernel decide a result.  Expected values come from
binning_cases.expected_scatter / expected_occ and oracle.voxel_oracle only.  No test lives here."""
from typing import NamedTuple, Optional, Tuple

import numpy as np

import binning_cases as bc
from oracle import voxel_oracle as vo


class Plan(NamedTuple):
    """sn_voxel_occupancy_plan's eight words."""
    one_pass: int
    slabs: int
    parts: int
    proof: int       # 0 none, 1 on the merged words, 2 second pass
    vec4: int
    wpr: int
    blocks: int      # finalize workgroups per tile
    lds: int         # dynamic LDS of the binning launch, bytes


class Case(NamedTuple):
    name: str
    dims: Tuple[int, int, int]        # (nx, ny, nz)
    fork: str                         # what the grid is there for
    plan1: Optional[Plan]             # one plane; None: SN_ERR_UNSUPPORTED
    plan2: Optional[Plan]             # with the tower plane
    fused: int = 0                    # 1: through sn_voxel_occupancy_fused (own box; the one-pass kernel where eligible)
    ws_aligned: int = 1


# lds = 8 * ((nx + ny + nz + 3 + 1) & ~1) + 4 * planes * words / slabs;  words = nx * ny * nz / 32;  wpr = ny // 32;
# blocks = ceil((words / 4 if words % 4 == 0 and the workspace is 16-byte aligned else words) / 256), at most
# ceil(2048 / B) -- no batch here has more than 32 tiles, and no grid asks for more than 128 blocks;
# parts = 16 / slabs (8 for the one-pass kernel).

# ---- the forks of occ_finalize_kernel, through sn_voxel_occupancy with a descriptor from bounds
FINALIZE = [
    Case("4x32x2", (4, 32, 2), "second pass, wpr 1 (8 words: no whole wave)",
         Plan(0, 1, 16, 2, 1, 1, 1, 368), Plan(0, 1, 16, 2, 1, 1, 1, 400)),
    Case("3x40x8", (3, 40, 8), "second pass from the word loop, rows straddle words at every offset",
         Plan(0, 1, 16, 2, 0, 1, 1, 552), Plan(0, 1, 16, 2, 0, 1, 1, 672)),
    Case("8x96x8", (8, 96, 8), "wpr 3: second pass under vec4",
         Plan(0, 1, 16, 2, 1, 3, 1, 1696), Plan(0, 1, 16, 2, 1, 3, 1, 2464)),
    Case("16x32x8", (16, 32, 8), "fused, wpr 1",
         Plan(0, 1, 16, 1, 1, 1, 1, 992), Plan(0, 1, 16, 1, 1, 1, 1, 1504)),
    Case("8x64x4", (8, 64, 4), "fused, wpr 2",
         Plan(0, 1, 16, 1, 1, 2, 1, 896), Plan(0, 1, 16, 1, 1, 2, 1, 1152)),
    Case("64x64x64", (64, 64, 64), "fused, wpr 2: the production grid, 8 finalize blocks",
         Plan(0, 1, 16, 1, 1, 2, 8, 34336), Plan(0, 1, 16, 1, 1, 2, 8, 67104)),
    Case("4x128x4", (4, 128, 4), "fused, wpr 4",
         Plan(0, 1, 16, 1, 1, 4, 1, 1376), Plan(0, 1, 16, 1, 1, 4, 1, 1632)),
    Case("4x256x2", (4, 256, 2), "fused, wpr 8, word loop with shuffles (words % 256 != 0)",
         Plan(0, 1, 16, 1, 0, 8, 1, 2384), Plan(0, 1, 16, 1, 0, 8, 1, 2640)),
    Case("4x256x8", (4, 256, 8), "fused, wpr 8, vec4 with one shuffle",
         Plan(0, 1, 16, 1, 1, 8, 1, 3200), Plan(0, 1, 16, 1, 1, 8, 1, 4224)),
    Case("2x512x8", (2, 512, 8), "fused, wpr 16, vec4 with two shuffles",
         Plan(0, 1, 16, 1, 1, 16, 1, 5232), Plan(0, 1, 16, 1, 1, 16, 1, 6256)),
    Case("1x2048x3", (1, 2048, 3), "fused, wpr 64, word loop: a whole wave per row",
         Plan(0, 1, 16, 1, 0, 64, 1, 17216), Plan(0, 1, 16, 1, 0, 64, 1, 17984)),
    Case("2x2048x2", (2, 2048, 2), "fused, wpr 64, vec4: sixteen lanes per row",
         Plan(0, 1, 16, 1, 1, 64, 1, 17472), Plan(0, 1, 16, 1, 1, 64, 1, 18496)),
    Case("2x4096x2", (2, 4096, 2), "wpr 128 > 64: second pass",
         Plan(0, 1, 16, 2, 1, 128, 1, 34880), Plan(0, 1, 16, 2, 1, 128, 1, 36928)),
]

# ---- the same kernels on a workspace that is only 4-byte aligned (one word into a larger buffer): vec4 off where it is
# otherwise on, so the fused proof of short rows runs in the word loop (o = wpr >> 1 ... 1) and the finalize grid is sized
# by words, not words / 4
UNALIGNED_WS = [
    Case("16x32x8-ws4", (16, 32, 8), "fused, wpr 1, word loop (workspace 4-byte aligned)",
         Plan(0, 1, 16, 1, 0, 1, 1, 992), Plan(0, 1, 16, 1, 0, 1, 1, 1504), ws_aligned=0),
    Case("8x64x4-ws4", (8, 64, 4), "fused, wpr 2, word loop (workspace 4-byte aligned)",
         Plan(0, 1, 16, 1, 0, 2, 1, 896), Plan(0, 1, 16, 1, 0, 2, 1, 1152), ws_aligned=0),
    Case("4x128x4-ws4", (4, 128, 4), "fused, wpr 4, word loop (workspace 4-byte aligned)",
         Plan(0, 1, 16, 1, 0, 4, 1, 1376), Plan(0, 1, 16, 1, 0, 4, 1, 1632), ws_aligned=0),
    Case("4x256x8-ws4", (4, 256, 8), "fused, wpr 8, word loop at words % 256 == 0 (workspace 4-byte aligned)",
         Plan(0, 1, 16, 1, 0, 8, 1, 3200), Plan(0, 1, 16, 1, 0, 8, 1, 4224), ws_aligned=0),
]

# ---- z-slabs at the LDS limit (B = 2), through sn_voxel_occupancy; None: the slab rule finds no plan
SLABS = [
    Case("64x64x128", (64, 64, 128), "words == 16384 exactly: one slab with one plane, two with the tower plane",
         Plan(0, 1, 16, 1, 1, 2, 16, 67616), Plan(0, 2, 8, 1, 1, 2, 16, 67616)),
    Case("64x128x96", (64, 128, 96), "two slabs of 48 planes: nz not a power of two",
         Plan(0, 2, 8, 1, 1, 4, 24, 51488), Plan(0, 4, 4, 1, 1, 4, 24, 51488)),
    Case("64x128x128", (64, 128, 128), "two slabs, four with the tower plane",
         Plan(0, 2, 8, 1, 1, 4, 32, 68128), Plan(0, 4, 4, 1, 1, 4, 32, 68128)),
    Case("128x128x256", (128, 128, 256), "eight slabs; sixteen with the tower plane: one workgroup per slab streams the tile",
         Plan(0, 8, 2, 1, 1, 4, 128, 69664), Plan(0, 16, 1, 1, 1, 4, 128, 69664)),
    Case("64x128x65", (64, 128, 65), "V % 32 == 0 and 16640 words, but no power-of-two slab count divides nz = 65", None, None),
]

# ---- the one-pass kernel (sn_voxel_occupancy_fused, option voxel_onepass = 1; with 0 the plan is plan?._replace(one_pass=0,
# parts=16))
ONEPASS = [
    Case("4x4x8-fused", (4, 4, 8), "one-pass, 4 words: a bitmap far smaller than the workgroup",
         Plan(1, 1, 8, 2, 1, 0, 1, 176), Plan(1, 1, 8, 2, 1, 0, 1, 192), fused=1),
    Case("16x32x8-fused", (16, 32, 8), "one-pass, 128 words: fewer than the workgroup's 1024 threads",
         Plan(1, 1, 8, 1, 1, 1, 1, 992), Plan(1, 1, 8, 1, 1, 1, 1, 1504), fused=1),
    Case("64x64x64-fused", (64, 64, 64), "one-pass, the production grid",
         Plan(1, 1, 8, 1, 1, 2, 8, 34336), Plan(1, 1, 8, 1, 1, 2, 8, 67104), fused=1),
    Case("64x64x128-fused", (64, 64, 128), "one-pass at the LDS limit (64 KiB bitmap); the tower plane needs two slabs: two-kernel form",
         Plan(1, 1, 8, 1, 1, 2, 16, 67616), Plan(0, 2, 8, 1, 1, 2, 16, 67616), fused=1),
]

ALL_CASES = FINALIZE + UNALIGNED_WS + SLABS + ONEPASS


def wpr_class(plan):
    """The class of ny / 32 the finalize kernel distinguishes (the ISSUE's list)."""
    w = plan.wpr
    if w > 64:
        return ">64"
    if w & (w - 1) or w == 0:
        return "not a power of two"
    if w >= 8:
        return "8..64 vec4" if plan.vec4 else "8..64 word loop"
    return str(w)


def fork_of(plan):
    """The name of a reachable fork: (proof, vec4, wpr class)."""
    return ("none", "fused", "second pass")[plan.proof], ("word loop", "vec4")[plan.vec4], wpr_class(plan)


# every (proof, loop, wpr class) occ_finalize_kernel can reach with flags given: a fused proof needs a power-of-two wpr
# <= 64; with vec4 and wpr >= 8 also words % 256 == 0
REQUIRED_FORKS = {("second pass", "vec4", "1"), ("second pass", "word loop", "1"),
                  ("second pass", "vec4", "not a power of two"), ("second pass", "vec4", ">64"),
                  ("fused", "vec4", "1"), ("fused", "vec4", "2"), ("fused", "vec4", "4"),
                  ("fused", "word loop", "1"), ("fused", "word loop", "2"), ("fused", "word loop", "4"),
                  ("fused", "vec4", "8..64 vec4"), ("fused", "word loop", "8..64 word loop")}
REQUIRED_SLABS = {1, 2, 4, 8, 16}

# the one-pass kernel's register budget is 7 pairs x 2 x 8 parts x 1024 threads = 114 688 points.  In this order, as one
# ragged batch, the tiles start at 0, 1, 3, 6, 1029, 17412, 33796, 50181, 164868, 279556, 394245, 508936: an even start
# meets odd and even lengths (1, 16384), an odd start too (3, 2); 114691 starts odd (aligned form: a lone first point and
# one surplus pair), 131073 starts even (a lone last point behind 8192 surplus pairs), 114689 fills the budget exactly
ONEPASS_SIZES = [1, 2, 3, 1023, 16383, 16384, 16385, 114687, 114688, 114689, 114691, 131073]
ONEPASS_BUDGET = 114688


# ---------------------------------------------------------------- a cloud from a prescribed count grid
def cloud_from_counts(desc_row, dims, counts, towers=None, n_outside=5, seed=0):
    """counts[nz, nx, ny] points at the centres of the cells of descriptor row `desc_row`, the first towers[cell] of each
    cell labelled 15.0 (kept), the rest 2.0 or 7.0 (not kept); n_outside points beyond the table (above the last edge of an
    axis, +inf, NaN: dropped) with labels from bc.LABELS.  Shuffled.  Returns (pts [N, 3], labels [N])."""
    nx, ny, nz = dims
    rng = np.random.default_rng(77 + seed)
    counts = np.asarray(counts, dtype=np.int64)
    assert counts.shape == (nz, nx, ny) and counts.min() >= 0
    towers = np.zeros_like(counts) if towers is None else np.asarray(towers, dtype=np.int64)
    assert towers.shape == counts.shape and (towers <= counts).all() and towers.min() >= 0
    (ex, ey, ez), _ = bc.tables_of(desc_row, dims)
    cx, cy, cz = [(e[:-1] + e[1:]) / 2 for e in (ex, ey, ez)]
    iz, ix, iy = np.nonzero(counts)
    c = counts[iz, ix, iy]
    rep = np.repeat(np.arange(len(c)), c)
    pts = np.stack([cx[ix][rep], cy[iy][rep], cz[iz][rep]], axis=1)
    k = np.arange(len(rep)) - np.repeat(np.cumsum(c) - c, c)           # rank of a point within its cell
    lab = np.where(k < towers[iz, ix, iy][rep], 15.0, np.where(k % 2 == 0, 2.0, 7.0))
    lo, hi = np.asarray(desc_row[:3]), np.asarray(desc_row[3:6])
    out = lo + rng.random((n_outside, 3)) * (hi - lo)
    for j in range(n_outside):
        out[j, j % 3] = (hi[j % 3] + (hi - lo)[j % 3], np.inf, np.nan)[(j // 3) % 3]
    pts = np.concatenate([pts, out])
    lab = np.concatenate([lab, bc.LABELS[rng.integers(0, len(bc.LABELS), n_outside)]])
    order = rng.permutation(len(pts))
    return pts[order], lab[order]


# ---------------------------------------------------------------- tile recipes
def boundary_rows(plan, rows):
    """Rows where the emptiness proof changes hands: first, second, around the middle, last two, and the last row one wave
    (and one 256-thread workgroup) of the finalize loop handles with the first row of the next.  A wave's 64 lanes hold
    64 rows in the second pass (a thread per row), else 64 words (256 with vec4) = that many / wpr rows."""
    per_wave = 64 if plan.proof != 1 else max(1, 64 * (4 if plan.vec4 else 1) // plan.wpr)
    want = [0, 1, rows // 2 - 1, rows // 2, rows - 2, rows - 1, per_wave - 1, per_wave, 4 * per_wave - 1, 4 * per_wave]
    return sorted({r for r in want if 0 <= r < rows})


def point_columns(ny):
    """y of the single point recipe C leaves in the row: first and last voxel, and bit 0 / bit 31 of the row's words 0, 1,
    wpr/2 - 1, wpr/2 and wpr - 1 where the row has two whole words or more."""
    ys = {0, ny - 1}
    wpr = ny // 32
    if ny % 32 == 0 and wpr >= 2:
        for k in (0, 1, wpr // 2 - 1, wpr // 2, wpr - 1):
            ys.update((32 * k, 32 * k + 31))
    return sorted(y for y in ys if 0 <= y < ny)


def recipe_tiles(case):
    """The count (and tower) grids of one call for `case`, as tiles of one batch: [(recipe name, counts, towers)].
    A   full: every (z, x) row holds a point, column y* holds one in every row, some of its cells exactly the column minimum
    E   sparse, LiDAR-like (the lower half of z only): between two flagged tiles
    D   A, whose tower plane has empty rows
    B-r A with row r emptied, r in boundary_rows
    C-y A with row r emptied but for one point at y, y in point_columns (r cycles through boundary_rows)"""
    nx, ny, nz = case.dims
    rows, V = nx * nz, nx * ny * nz
    rng = np.random.default_rng(4242 + V)
    p = min(0.3, 2000.0 / V)
    ystar = ny // 3

    def full():
        c = (rng.random((rows, ny)) < p) * rng.integers(1, 4, (rows, ny))
        col = 1 + rng.integers(0, 3, rows)
        col[rng.integers(0, rows)] = 1          # the column minimum is 1 ...
        col[(int(np.argmin(col)) + 1) % rows] = 3   # ... and some cell is above it
        c[:, ystar] = col
        t = np.minimum(c, rng.integers(0, 3, (rows, ny)))
        return c, t

    tiles = []
    a, t = full()
    tiles.append(("A", a, t))
    e = np.zeros((rows, ny), dtype=np.int64)
    half = rows // 2                                   # (every grid of the table has three rows or more)
    e[:half] = (rng.random((half, ny)) < p) * rng.integers(1, 4, (half, ny))
    tiles.append(("E", e, np.minimum(e, 1)))
    d, t = full()
    t[::2] = 0
    tiles.append(("D", d, t))
    plan = case.plan1
    brows = boundary_rows(plan, rows)
    for r in brows:
        b, t = full()
        b[r] = 0
        t[r] = 0
        tiles.append((f"B-{r}", b, t))
    for i, y in enumerate(point_columns(ny)):
        r = brows[i % len(brows)]
        c, t = full()
        c[r] = 0
        c[r, y] = 1
        t[r] = 0
        tiles.append((f"C-{y}", c, t))
    return [(n, c.reshape(nz, nx, ny), t.reshape(nz, nx, ny)) for n, c, t in tiles]


def expected_flags(counts):
    """A tile's flag stays up iff none of its (z, x) rows is empty."""
    return (np.asarray(counts).sum(axis=-1) > 0).all(axis=(-2, -1)).astype(np.int64)


def recipe_batch(case):
    """(host desc [B, len], tiles, labels, names, count grids [B, nz, nx, ny], tower grids) of recipe_tiles(case), each tile
    in its own caller-given box (bc.bounds_box)."""
    recipes = recipe_tiles(case)
    B = len(recipes)
    desc, _ = bc.host_desc("bounds", case.dims, B)
    tiles, labels = [], []
    for b, (_, c, t) in enumerate(recipes):
        pts, lab = cloud_from_counts(desc[b], case.dims, c, t, n_outside=3 + b % 7, seed=b)
        tiles.append(pts)
        labels.append(lab)
    return (desc, tiles, labels, [n for n, _, _ in recipes], np.stack([c for _, c, _ in recipes]),
            np.stack([t for _, _, t in recipes]))


# ---------------------------------------------------------------- slabs
def slab_batch(case, planes, B=2, n_random=3000):
    """B tiles for a z-slab grid: n_random uniform points in the box (some outside: dropped), and a point in the last voxel
    of every slab and the first of the next (every x, y corner), labels from bc.LABELS.  Returns (host desc, tiles, labels)."""
    nx, ny, nz = case.dims
    plan = case.plan2 if planes == 2 else case.plan1
    slabs = plan.slabs if plan is not None else 1
    desc, _ = bc.host_desc("bounds", case.dims, B)
    tiles, labels = [], []
    for b in range(B):
        rng = np.random.default_rng(600 + b)
        lo, hi = desc[b, :3], desc[b, 3:6]
        rnd = (lo - 0.05 * (hi - lo)) + rng.random((n_random, 3)) * (1.1 * (hi - lo))
        (ex, ey, ez), _ = bc.tables_of(desc[b], case.dims)
        cx, cy, cz = [(e[:-1] + e[1:]) / 2 for e in (ex, ey, ez)]
        zs = sorted({z for s in range(1, slabs) for z in (s * (nz // slabs) - 1, s * (nz // slabs))} | {0, nz - 1})
        seam = np.array([[cx[i], cy[j], cz[z]] for z in zs for i in (0, nx - 1) for j in (0, ny - 1)])
        pts = np.concatenate([rnd, seam])
        rng.shuffle(pts, axis=0)
        tiles.append(pts)
        labels.append(bc.LABELS[rng.integers(0, len(bc.LABELS), len(pts))])
    return desc, tiles, labels


# ---------------------------------------------------------------- own-box descriptors (the fused entry)
def own_box_counts(xyz, dims, labels, keep, regular):
    """counts, towers [nz, nx, ny], the descriptor row (lo, hi, edges) and the raw box of a tile voxelised in its own box:
    oracle.voxel_oracle.voxelgrid_compute with the cube (`regular`) or with the box as it is (regular_bounding_box=False:
    edges numpy.linspace(min, max, n + 1) per axis)."""
    nx, ny, nz = dims
    g = vo.voxelgrid_compute(xyz, n_xyz=dims, regular_bounding_box=bool(regular))
    vx, vy, vz = g["voxel_x"], g["voxel_y"], g["voxel_z"]
    assert (vx < nx).all() and (vy < ny).all() and (vz < nz).all()
    flat = (vz * nx + vx) * ny + vy
    counts = np.bincount(flat, minlength=nz * nx * ny).reshape(nz, nx, ny)
    kept = np.isin(np.asarray(labels), np.asarray(keep))
    towers = np.bincount(flat[kept], minlength=nz * nx * ny).reshape(nz, nx, ny)
    desc = np.concatenate([g["xyzmin"], g["xyzmax"]] + list(g["segments"]))
    bbox = np.concatenate([np.asarray(xyz).min(0), np.asarray(xyz).max(0)])
    return counts, towers, desc, bbox


def onepass_tiles(seed=11):
    """One ragged batch of ONEPASS_SIZES: clouds at UTM scale, another extent per tile, labels from bc.LABELS."""
    tiles, labels = [], []
    for t, n in enumerate(ONEPASS_SIZES):
        rng = np.random.default_rng(seed + t)
        ext = np.array([31.0, 23.0, 11.0]) * (1.0 + 0.1 * t)
        # (a bell in x and y, thin in z: most voxels stay empty, so no tile of the production grid is flagged)
        u = np.clip(rng.normal(0.5, 0.18, (n, 3)), 0.0, 1.0)
        u[:, 2] = rng.random(n) ** 3
        tiles.append(bc.UTM + 17.0 * t + u * ext)
        labels.append(bc.LABELS[rng.integers(0, len(bc.LABELS), n)])
    return tiles, labels


# ---------------------------------------------------------------- counting path
COUNTING_DIMS = [(2, 300, 3),     # a second y0 trip of 44 columns: 5 row lanes deep, 36 threads idle
                 (2, 257, 3),     # a second trip of one column: 256 row lanes for 6 rows
                 (2, 256, 3),     # exactly one trip
                 (3, 100, 2)]     # one trip, 2 row lanes, 56 threads idle


def counting_grids(dims):
    """Three count grids [nz, nx, ny] for the counting path: sparse; every cell >= 1 (the column minima are nonzero in
    every y0 trip), with a few columns constant; one row only."""
    nx, ny, nz = dims
    rng = np.random.default_rng(sum(dims))
    sparse = (rng.random((nz, nx, ny)) < 0.3) * rng.integers(1, 5, (nz, nx, ny))
    dense = rng.integers(1, 6, (nz, nx, ny))
    dense[:, :, ::7] = 2
    dense[0, 0, :] = dense.min(axis=(0, 1))           # a cell at the column minimum in every column
    one_row = np.zeros((nz, nx, ny), dtype=np.int64)
    one_row[nz - 1, nx - 1] = rng.integers(0, 3, ny)
    grids = [sparse, dense, one_row]
    return grids, [np.minimum(g, rng.integers(0, 3, g.shape)) for g in grids]
