"""The shapes of test_gpu_corr_plans.py and the fork of the backward correlation (sn_conv_corr_ws: csrc/corr.hip,
csrc/backward.hip) each one is there for.  test_corr_plan_host.py asks the library's plan query (sn_conv_corr_plan) for
every row on any machine, so a planner change that moves a shape off its fork fails without a device; the GPU test asks it
again before every launch.

A fork is a dict of CorrPlan fields (scene_net_amd._hip) and their wanted values, plus two derived ones:
    many_jobs   workgroups < jobs: a persistent workgroup takes a second job
    row_tiled   more than one row tile per plane"""
from typing import NamedTuple

DENSE = {"corr_dense": 1}


def gather(tile_bytes=0):
    return {"corr_dense": 0, "corr_sparse_tile_bytes": tile_bytes}


class Case(NamedTuple):
    shape: tuple     # [B,1,Z,X,Y]
    ks: tuple
    opts: dict
    fork: dict


GATHER, GEMM, TAPS = "gather", "gemm", "taps"

MANY_JOBS = {
    "gather_3x3x3_tile8": Case((2, 1, 50, 8, 8), (3, 3, 3), gather(8), dict(kernel=GATHER, rows=1, many_jobs=True, list_vec=True)),
    "gather_5x3x5_tile12": Case((3, 1, 40, 9, 12), (5, 3, 5), gather(12), dict(kernel=GATHER, rows=1, many_jobs=True, list_vec=False)),
    "gather_9x9x9_tile20": Case((7, 1, 40, 10, 20), (9, 9, 9), gather(20), dict(kernel=GATHER, rows=1, many_jobs=True, multi_group=True)),
    "gemm_3x3x3": Case((13, 1, 64, 8, 8), (3, 3, 3), DENSE, dict(kernel=GEMM, many_jobs=True, row_tiled=False)),
}

GEMM_TILES = {
    "two_row_tiles_80_steps": Case((1, 1, 6, 60, 300), (3, 3, 5), DENSE, dict(kernel=GEMM, rows=56, row_tiled=True, every_step=True)),
    "two_row_tiles_many_jobs": Case((22, 1, 6, 60, 300), (3, 3, 5), DENSE,
                                    dict(kernel=GEMM, rows=56, row_tiled=True, every_step=True, many_jobs=True)),
    "one_tile_40_steps": Case((1, 1, 6, 60, 132), (3, 3, 5), DENSE, dict(kernel=GEMM, row_tiled=False, every_step=True)),
    # Y = 1700: one row and its halo overflow the gather's 3072-element delta tile; the GEMM form takes it, 8 rows a job
    "gather_refuses_y1700": Case((1, 1, 3, 9, 1700), (3, 3, 3), gather(0), dict(kernel=GEMM, rows=8, row_tiled=True, every_step=True)),
}

KZ16 = {
    "kz11": ((1, 1, 12, 10, 16), (11, 3, 5)),
    "kz16": ((1, 1, 20, 9, 12), (16, 5, 4)),
}

EXTENT_SHAPE = (1, 1, 5, 12, 16)
EXTENTS_BOTH = [(1, 1, 1), (3, 16, 16), (3, 1, 16), (3, 16, 1)]     # through the gather and through the GEMM form
EXTENTS_WIDE = [(3, 17, 17), (3, 20, 20)]                           # the gather (one group, idle threads) and the fallback

TAPS_TILES = {
    # two tiles of the thread-per-tap kernel (8 x 8 x 64) along each axis
    "two_tiles_per_axis": Case((2, 1, 11, 13, 70), (3, 3, 17), DENSE, dict(kernel=TAPS, row_tiled=True, jobs=16)),
    # extents <= 16, but 8 rows of Y = 2200 do not fit the GEMM form's LDS tile
    "no_gemm_plan": Case((1, 1, 2, 3, 2200), (3, 3, 3), DENSE, dict(kernel=TAPS, jobs=35)),
}

# exact impulse tests: (shape, ks, options, fork); the row-tile seam is taken from the plan's `rows`
IMPULSE = {
    "gather_default_tile": Case((3, 1, 5, 70, 32), (3, 3, 3), gather(0), dict(kernel=GATHER, row_tiled=True)),
    "gather_one_row_tiles": Case((3, 1, 5, 70, 32), (3, 3, 3), gather(32), dict(kernel=GATHER, rows=1, many_jobs=True)),
    "gemm_row_tiled": Case((1, 1, 6, 60, 300), (3, 3, 5), DENSE, dict(kernel=GEMM, row_tiled=True, every_step=True)),
    "gemm_many_jobs": Case((13, 1, 64, 8, 8), (3, 3, 3), DENSE, dict(kernel=GEMM, many_jobs=True)),
    "taps": Case((2, 1, 11, 13, 70), (3, 3, 17), DENSE, dict(kernel=TAPS, row_tiled=True)),
}

# alignment: Y a multiple of 8, so every vector staging form is on until a pointer breaks it
ALIGN_SHAPE, ALIGN_KS = (2, 1, 6, 9, 16), (3, 5, 3)
# input types with the derivative: nothing a multiple of anything
RAGGED_SHAPE, RAGGED_KS = (2, 1, 7, 11, 13), (5, 3, 5)


MANY_JOBS_DENSITIES = (0.03, 0.6, "layered")     # layered: all empty but two z planes at density 0.5
TILES_DENSITIES = (0.01, 0.6)
SMALL_DENSITIES = (0.05, 0.5)


def bar_cases():
    """(shape, ks, densities) of every comparison with the fp64 reference: what tools/corr_bar_constant.py emulates to
    measure the constants of the elementwise bar"""
    rows = [(c.shape, c.ks, MANY_JOBS_DENSITIES) for c in MANY_JOBS.values()]
    rows += [(c.shape, c.ks, TILES_DENSITIES[:1] if c.shape[0] > 1 else TILES_DENSITIES) for c in GEMM_TILES.values()]
    rows += [(shape, ks, SMALL_DENSITIES) for shape, ks in KZ16.values()]
    rows += [(EXTENT_SHAPE, ks, SMALL_DENSITIES) for ks in EXTENTS_BOTH + EXTENTS_WIDE]
    rows += [(c.shape, c.ks, SMALL_DENSITIES) for c in TAPS_TILES.values()]
    rows += [(ALIGN_SHAPE, ALIGN_KS, SMALL_DENSITIES), (RAGGED_SHAPE, RAGGED_KS, SMALL_DENSITIES)]
    return rows


def fork_misses(plan, fork):
    """the entries of `fork` that `plan` (a CorrPlan) does not meet; empty when the shape is on its fork"""
    bad = {}
    for key, want in fork.items():
        if key == "many_jobs":
            got = plan.workgroups < plan.jobs
        elif key == "row_tiled":
            got = plan.row_tiles > 1
        else:
            got = getattr(plan, key)
        if got != want:
            bad[key] = (got, want)
    return bad


def all_cases():
    """name -> (x dtype name, g dtype name, Case) for every row above, the way the GPU test launches it"""
    rows = {}
    for table in (MANY_JOBS, GEMM_TILES, TAPS_TILES, IMPULSE):
        for name, case in table.items():
            rows[name] = ("bool", "float32", case)
    for name, (shape, ks) in KZ16.items():
        for g in ("float32", "bfloat16"):
            rows[f"{name}_gather_{g}"] = ("bool", g, Case(shape, ks, gather(0), dict(kernel=GATHER, kzmax=16)))
            rows[f"{name}_gemm_{g}"] = ("bool", g, Case(shape, ks, DENSE, dict(kernel=GEMM, kzmax=16)))
    for ks in EXTENTS_BOTH:
        tag = "x".join(map(str, ks))
        rows[f"extent_{tag}_gather"] = ("bool", "float32", Case(EXTENT_SHAPE, ks, gather(0),
                                                                 dict(kernel=GATHER, kzmax=9, multi_group=True)))
        rows[f"extent_{tag}_gemm"] = ("bool", "float32", Case(EXTENT_SHAPE, ks, DENSE, dict(kernel=GEMM, kzmax=9)))
    for ks in EXTENTS_WIDE:
        tag = "x".join(map(str, ks))
        rows[f"extent_{tag}_gather"] = ("bool", "float32", Case(EXTENT_SHAPE, ks, gather(0),
                                                                 dict(kernel=GATHER, multi_group=False)))
        rows[f"extent_{tag}_taps"] = ("bool", "float32", Case(EXTENT_SHAPE, ks, DENSE, dict(kernel=TAPS, kzmax=0)))
    for x in ("float32", "float64", "uint8", "bool"):
        rows[f"ragged_gemm_{x}"] = (x, "float32", Case(RAGGED_SHAPE, RAGGED_KS, DENSE, dict(kernel=GEMM, vec=False)))
        rows[f"align_gemm_{x}"] = (x, "float32", Case(ALIGN_SHAPE, ALIGN_KS, DENSE, dict(kernel=GEMM, vec=True)))
    rows["align_gather"] = ("bool", "float32", Case(ALIGN_SHAPE, ALIGN_KS, gather(0),
                                                    dict(kernel=GATHER, vec=True, list_vec=True)))
    return rows
