"""The helper of the foreign-point binning tests (tests/binning_cases.py) on the CPU: its rule is the oracle's on a tile's
own points, and the point sets the GPU tests bin are not vacuous -- each holds its share of points outside the table, of
points clipped into bin 0, of plainly inside points and of NaN rows."""
import numpy as np
import pytest

import binning_cases as bc
from oracle import voxel_oracle as vo

CASES = [(k, d) for k in ("own", "bounds") for d in bc.DIMS + [bc.SLAB_DIMS]] + [("sized", bc.CAPACITY)]


@pytest.mark.parametrize("dims", bc.DIMS)
def test_rule_is_the_oracle_on_a_tiles_own_points_n_mode(dims):
    """expected_flat == voxelgrid_compute's indices (np.searchsorted - 1, clipped) where both are defined: the points the
    table was built from, the box's corners (p == e_0 and p == e_n) among them."""
    nx, ny, nz = dims
    desc, _ = bc.host_desc("own", dims, 3)
    for b in range(3):
        cloud = bc.own_cloud(b)
        g = vo.voxelgrid_compute(cloud, n_xyz=dims)
        assert np.array_equal(desc[b, :3], g["xyzmin"]) and np.array_equal(desc[b, 6:], np.concatenate(g["segments"]))
        want = (g["voxel_z"] * nx + g["voxel_x"]) * ny + g["voxel_y"]
        got = bc.expected_flat(desc[b], dims, cloud)
        assert (got >= 0).all() and np.array_equal(got, want)
        counts, _, dropped = bc.expected_scatter(desc[b:b + 1], dims, [cloud])
        assert np.array_equal(counts[0], vo.voxel_counts(cloud, dims)[0]) and dropped[0] == 0


def test_rule_is_the_oracle_on_a_tiles_own_points_size_mode():
    """the same on the padded per-tile tables of the size mode, whose own dims differ per tile and stay below the capacity"""
    nx, ny, nz = bc.CAPACITY
    desc, own = bc.host_desc("sized", bc.CAPACITY, 4)
    assert len({tuple(o) for o in own.tolist()}) == 4 and (own < np.array(bc.CAPACITY)).all() and (own > 4).all()
    for b in range(4):
        cloud = bc.own_cloud(b)
        g = vo.voxelgrid_compute(cloud, sizes=bc.VOXEL_SIZE)
        assert own[b].tolist() == [int(v) for v in g["x_y_z"]]
        want = (g["voxel_z"] * nx + g["voxel_x"]) * ny + g["voxel_y"]
        assert np.array_equal(bc.expected_flat(desc[b], bc.CAPACITY, cloud, own[b]), want)
        # on its own points the padded table gives the same answer with and without the cut to the tile's dims
        assert np.array_equal(bc.expected_flat(desc[b], bc.CAPACITY, cloud), want)
        (ex, ey, ez), _ = bc.tables_of(desc[b], bc.CAPACITY)
        for e, n in zip((ex, ey, ez), own[b]):
            assert np.isfinite(e[:n + 1]).all() and np.isinf(e[n + 1:]).all()


def test_rule_at_the_ends_of_a_table():
    """below the box clips to bin 0 (-inf included), e_n is the last bin, anything above it and NaN is outside; on a padded
    table the tile's OWN last edge decides, not the capacity's"""
    e = vo.linspace_edges(0.0, 8.0, 5)
    p = np.array([-np.inf, -1e300, -1.0, 0.0, np.nextafter(0.0, 1.0), e[1], np.nextafter(e[1], 9.0), 8.0,
                  np.nextafter(8.0, 9.0), 9.0, 1e9, 1e300, np.inf, np.nan])
    assert bc.axis_index(e, p).tolist() == [0, 0, 0, 0, 0, 0, 1, 4, 5, 5, 5, 5, 5, 5]
    padded = np.concatenate([[0.0] * 3, [8.0] * 3] + [np.concatenate([e, [np.inf] * 3])] * 3)
    pts = np.stack([p, np.full_like(p, 4.0), np.full_like(p, 4.0)], axis=1)
    own = bc.expected_flat(padded, (8, 8, 8), pts, (5, 5, 5))
    assert (own[8:] == -1).all() and (own[:8] >= 0).all()
    # without the cut the padding cell n_a = 5 takes them: what the kernels' Binner::flat computes on a padded table
    assert (bc.expected_flat(padded, (8, 8, 8), pts)[8:13] == (2 * 8 + 5) * 8 + 2).all()


@pytest.mark.parametrize("kind,dims", CASES, ids=[f"{k}-{'x'.join(map(str, d))}" for k, d in CASES])
def test_the_gpu_tests_point_sets_are_not_vacuous(kind, dims):
    """for every (box, dims) of tests/test_gpu_binning_foreign.py: >= 20 % of the points outside the table, >= 20 % clipped
    low on some axis without being outside, >= 20 % plainly inside, >= 6 rows with a NaN -- per full foreign set and over
    the batch; the one-point tile's point is outside, the first tile has 1001 points (an odd start for the next)"""
    desc, own = bc.host_desc(kind, dims, 4)
    tiles, labels = bc.foreign_batch(desc, dims, own)
    assert [len(t) for t in tiles[:2]] == [1001, 1] and 1000 <= len(tiles[2]) <= 5000
    assert all(len(l) == len(t) for l, t in zip(labels, tiles))
    o = lambda b: None if own is None else own[b]   # noqa: E731
    assert bc.expected_flat(desc[1], dims, tiles[1], o(1)).tolist() == [-1]
    for b in (0, 2):
        out, low, inside, nan_rows = bc.shares(desc[b], dims, tiles[b], o(b))
        assert out >= 0.2 and low >= 0.2 and inside >= 0.2, (out, low, inside)
        assert abs(out + low + inside - 1.0) < 1e-12
        if b == 2:
            assert nan_rows >= 6
    counts, towers, dropped = bc.expected_scatter(desc, dims, tiles, labels, own=own)
    assert (counts.sum(axis=(1, 2, 3)) + dropped).tolist() == [len(t) for t in tiles]
    assert (towers <= counts).all() and 0 < towers.sum() < counts.sum() and dropped[1] == 1
    if own is not None:   # nothing lands beyond a tile's own dims
        for b in range(3):
            nxo, nyo, nzo = own[b]
            assert counts[b].sum() == counts[b, :nzo, :nxo, :nyo].sum()


def test_expected_gather_reads_each_tiles_own_grid():
    dims = (5, 7, 3)
    desc, _ = bc.host_desc("bounds", dims, 4)
    tiles, _ = bc.foreign_batch(desc, dims)
    tiles = tiles[:2] + [np.empty((0, 3))] + tiles[2:]
    V = 5 * 7 * 3
    grid = np.arange(4 * 3 * V, dtype=np.float64).reshape(4, 3, 3, 5, 7)
    got = bc.expected_gather(grid, desc, dims, tiles, np.nan)
    assert got.shape == (3, sum(len(t) for t in tiles))
    f = bc.expected_flat(desc[3], dims, tiles[3])
    tail = got[:, -len(f):]
    assert np.array_equal(np.isnan(tail[1]), f < 0)
    assert np.array_equal(tail[1][f >= 0], (3 * 3 + 1) * V + f[f >= 0])
    assert np.isnan(got[:, 1001]).all()          # the one-point tile's point is outside
