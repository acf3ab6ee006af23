"""The plan table and the constructions of tests/voxel_plan_cases.py, checked on the host (no GPU): the table reaches every
fork of K1's LDS-bitmap path, sn_voxel_occupancy_plan (host arithmetic) reports the hand-written words, the cloud builder
reproduces its count grids under the binning rule of tests/binning_cases.py, and the tile recipes are what the GPU file
needs them to be -- a recipe-A tile whose ToFullDense(normalize_xyz(counts)) equalled counts > 0 could not tell the exact
fallback from the bitmap."""
import numpy as np
import pytest

import binning_cases as bc
import voxel_plan_cases as pc
from scene_net_amd import _hip


def _plans(case):
    return [(1, case.plan1), (2, case.plan2)]


def test_the_table_reaches_every_fork():
    plans = [p for c in pc.ALL_CASES for _, p in _plans(c) if p is not None]
    forks = {pc.fork_of(p) for p in plans}
    for fork in sorted(pc.REQUIRED_FORKS):
        assert fork in forks, f"no case selects the finalize fork {fork}"
    for s in sorted(pc.REQUIRED_SLABS):
        assert s in {p.slabs for p in plans}, f"no case takes {s} z-slab(s)"
    assert {p.one_pass for p in plans} == {0, 1}, "one-pass and two-kernel forms"
    assert any(c.plan1 is None for c in pc.ALL_CASES), "no unsupported grid in the table"
    assert any(p.slabs == 16 and p.parts == 1 for p in plans), "slabs == 16: one workgroup per slab"
    assert any(p.slabs == 1 and p.lds - 8 * ((sum(c.dims) + 4) & ~1) == 65536 for c in pc.ALL_CASES for _, p in _plans(c)
               if p is not None), "a full 64 KiB bitmap in one slab"
    names = [c.name for c in pc.ALL_CASES]
    assert len(names) == len(set(names))


@pytest.mark.parametrize("case", pc.ALL_CASES, ids=[c.name for c in pc.ALL_CASES])
def test_plan_query_reports_the_table(case):
    """sn_voxel_occupancy_plan against the hand-written words; _hip.occupancy_supported agrees with the supported column.
    B = 2: no case's finalize grid reaches the ceil(2048 / B) cap."""
    for planes, want in _plans(case):
        got = _hip.voxel_occupancy_plan(case.dims, planes, 2, fused=bool(case.fused), ws_aligned16=bool(case.ws_aligned))
        assert (got is None) == (want is None), (planes, got)
        assert _hip.occupancy_supported(case.dims, planes) == (want is not None)
        if want is not None:
            assert tuple(got) == tuple(want), (planes, got, want)
            # no flags asked for: no proof, and nothing keeps the finalize kernel from four words per thread
            bare = _hip.voxel_occupancy_plan(case.dims, planes, 2, fused=bool(case.fused), ws_aligned16=bool(case.ws_aligned),
                                             want_flags=False)
            words = case.dims[0] * case.dims[1] * case.dims[2] // 32
            assert bare.proof == 0 and bare.vec4 == int(bool(case.ws_aligned) and words % 4 == 0)
            # voxel-size mode never rides the proof on the merged words, and never takes the one-pass kernel
            sized = _hip.voxel_occupancy_plan(case.dims, planes, 2, fused=True, sized=True, ws_aligned16=bool(case.ws_aligned))
            assert sized.proof == 2 and sized.one_pass == 0 and sized.slabs == want.slabs


def test_one_pass_follows_its_option():
    for case in pc.ONEPASS:
        for planes, want in _plans(case):
            with _hip.options(voxel_onepass=0):
                got = _hip.voxel_occupancy_plan(case.dims, planes, 2, fused=True)
            assert tuple(got) == tuple(want._replace(one_pass=0, parts=16 // want.slabs))
            # a descriptor given (sn_voxel_occupancy): never the one-pass kernel
            assert _hip.voxel_occupancy_plan(case.dims, planes, 2, fused=False).one_pass == 0


def test_finalize_grid_is_capped_by_the_batch():
    assert _hip.voxel_occupancy_plan((64, 64, 64), 1, 1).finalize_blocks == 8
    assert _hip.voxel_occupancy_plan((64, 64, 64), 1, 512).finalize_blocks == 4      # ceil(2048 / 512)
    assert _hip.voxel_occupancy_plan((128, 128, 256), 1, 16).finalize_blocks == 128
    assert _hip.voxel_occupancy_plan((128, 128, 256), 1, 4096).finalize_blocks == 1


RECIPE_CASES = pc.FINALIZE + pc.UNALIGNED_WS


@pytest.mark.parametrize("case", RECIPE_CASES, ids=[c.name for c in RECIPE_CASES])
def test_recipes_are_what_the_gpu_test_needs(case):
    desc, tiles, labels, names, counts, towers = pc.recipe_batch(case)
    c, t, dropped = bc.expected_scatter(desc, case.dims, tiles, labels)
    assert np.array_equal(c, counts) and np.array_equal(t, towers), "the cloud does not reproduce its count grid"
    assert dropped.tolist() == [3 + b % 7 for b in range(len(tiles))]
    flags = pc.expected_flags(c)
    occ = bc.expected_occ(c)
    assert names[:3] == ["A", "E", "D"]
    for b, n in enumerate(names):
        kind = n.split("-")[0]
        assert flags[b] == {"A": 1, "E": 0, "D": 1, "B": 0, "C": 1}[kind], n
        if kind in "AD":
            assert not np.array_equal(occ[b], c[b] > 0), f"{n}: the column rule does not matter for this tile"
        if kind == "D":
            assert (t[b].sum(axis=-1) == 0).any() and (t[b] > 0).any()
    rows = case.dims[0] * case.dims[2]
    assert sum(n[0] == "B" for n in names) == len(pc.boundary_rows(case.plan1, rows)) >= min(rows, 3)
    assert sum(n[0] == "C" for n in names) == len(pc.point_columns(case.dims[1])) >= 2
    assert len(tiles) <= 32


def test_boundary_rows_and_point_columns():
    by = {c.name: c for c in pc.FINALIZE}
    # 64^3, fused proof under vec4: a wave's 256 words are 128 rows, a workgroup's 1024 words 512
    assert pc.boundary_rows(by["64x64x64"].plan1, 4096) == [0, 1, 127, 128, 511, 512, 2047, 2048, 4094, 4095]
    assert pc.boundary_rows(by["1x2048x3"].plan1, 3) == [0, 1, 2]            # a whole wave per row
    assert pc.boundary_rows(by["3x40x8"].plan1, 24) == [0, 1, 11, 12, 22, 23]  # second pass: 64 rows per wave, 24 in all
    assert pc.boundary_rows(by["8x96x8"].plan1, 64) == [0, 1, 31, 32, 62, 63]
    assert pc.point_columns(40) == [0, 39]
    assert pc.point_columns(64) == [0, 31, 32, 63]
    assert pc.point_columns(256) == [0, 31, 32, 63, 96, 127, 128, 159, 224, 255]


def test_one_pass_sizes_meet_every_parity_and_the_budget():
    sizes = pc.ONEPASS_SIZES
    assert sorted(sizes) == [1, 2, 3, 1023, 16383, 16384, 16385, 114687, 114688, 114689, 114691, 131073]
    starts = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    assert {(int(s) & 1, n & 1) for s, n in zip(starts, sizes)} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    over = [(int(s) & 1, n) for s, n in zip(starts, sizes) if n > pc.ONEPASS_BUDGET]
    assert {p for p, _ in over} == {0, 1}, "the surplus stream with a lone first and with a lone last point"
    tiles, labels = pc.onepass_tiles()
    assert [len(t) for t in tiles] == sizes and all(len(l) == len(t) for t, l in zip(tiles, labels))


@pytest.mark.parametrize("dims", pc.COUNTING_DIMS, ids=["x".join(map(str, d)) for d in pc.COUNTING_DIMS])
def test_counting_grids(dims):
    grids, towers = pc.counting_grids(dims)
    assert grids[1].min() >= 1 and (grids[1].min(axis=(0, 1)) >= 1).all()       # nonzero minima in every y0 trip
    assert not np.array_equal(bc.expected_occ(np.stack(grids))[1], grids[1] > 0)
    desc, _ = bc.host_desc("bounds", dims, 3)
    for b, (g, t) in enumerate(zip(grids, towers)):
        pts, lab = pc.cloud_from_counts(desc[b], dims, g, t, n_outside=4, seed=b)
        c, tw, d = bc.expected_scatter(desc[b:b + 1], dims, [pts], [lab])
        assert np.array_equal(c[0], g) and np.array_equal(tw[0], t) and d[0] == 4


def test_own_box_counts_match_the_oracle_with_the_cube():
    from oracle import voxel_oracle as vo
    rng = np.random.default_rng(5)
    xyz = bc.UTM + rng.random((500, 3)) * [20.0, 9.0, 4.0]
    lab = bc.LABELS[rng.integers(0, 4, 500)]
    c, t, desc, bbox = pc.own_box_counts(xyz, (16, 32, 8), lab, bc.KEEP, True)
    c0, t0, g = vo.voxel_counts(xyz, (16, 32, 8), None, lab, bc.KEEP)
    assert np.array_equal(c, c0) and np.array_equal(t, t0) and np.array_equal(desc[:3], g["xyzmin"])
    c1, _, d1, _ = pc.own_box_counts(xyz, (16, 32, 8), lab, bc.KEEP, False)
    assert np.array_equal(d1[:3], xyz.min(0)) and np.array_equal(d1[3:6], xyz.max(0)) and c1.sum() == 500
    assert np.array_equal(d1[6:6 + 17], np.linspace(xyz[:, 0].min(), xyz[:, 0].max(), 17))
