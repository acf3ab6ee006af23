"""K24 without a GPU: the argument checks of sn_voxel_pool (they run before any launch), and the numpy restatement of its
rules (tests/voxel_pool_cases.py) against the fp64 mean it approximates -- the bound, the invariance under a permutation of
the rows, the one-point tile and the accounting of the rows."""
import ctypes

import numpy as np
import pytest

import binning_cases as bc
import voxel_pool_cases as pc
import scene_net_amd as sna
from scene_net_amd import _hip

KINDS = [("own", d) for d in bc.DIMS] + [("bounds", d) for d in bc.DIMS] + [("sized", bc.CAPACITY)]


def test_argument_checks_need_no_gpu():
    lib = _hip.load()
    buf = ctypes.create_string_buffer(256)
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert p.value % 8 == 0
    off = lambda k: ctypes.c_void_p(p.value + k)   # noqa: E731
    i32 = lambda *v: (ctypes.c_int32 * len(v))(*v)   # noqa: E731
    f64 = lambda *v: (ctypes.c_double * len(v))(*v)   # noqa: E731

    def pool(pts=p, values=p, C=2, offsets=p, total=100, B=2, desc=p, dims=(4, 4, 4), src=(0, 1, 2), op=(0, 0, 0), P=None,
             ranges=(0.0, 1.0, 0.0, 1.0), fill=0.0, flags=0, ws=None, out=p, counts=p, unbinned=p, nan_rows=p):
        P = len(src) if P is None else P
        return lib.sn_voxel_pool(pts, values, C, offsets, total, B, desc, *dims, i32(*src), i32(*op), P,
                                 None if ranges is None else f64(*ranges), fill, flags, ws, out, counts, unbinned,
                                 nan_rows, None)

    for name in ("pts", "offsets", "desc", "out", "counts", "unbinned", "nan_rows"):
        assert pool(**{name: None}) == -1, name
        assert b"null" in lib.sn_last_error(), name
        assert pool(**{name: off(2 if name == "counts" else 4)}) == -1, name
        assert b"aligned" in lib.sn_last_error(), name
    assert pool(values=off(4), src=(3,), op=(2,)) == -1 and b"aligned" in lib.sn_last_error()
    # values may be null while no plane reads a column, and not otherwise
    assert pool(values=None, src=(0, 3), op=(0, 2)) == -1 and b"values is null" in lib.sn_last_error()
    for kw in (dict(C=-1), dict(C=6)):
        assert pool(**kw) == -1 and b"C must be" in lib.sn_last_error()
    for kw in (dict(src=(), op=()), dict(src=(0,) * 9, op=(0,) * 9)):
        assert pool(**kw) == -1 and b"P must be" in lib.sn_last_error()
    for src in ((5,), (-1,), (0, 1, 7)):
        assert pool(src=src, op=(0,) * len(src)) == -1 and b"source" in lib.sn_last_error()
    assert pool(C=0, values=None, src=(3,), op=(0,)) == -1 and b"source" in lib.sn_last_error()
    for op in ((3,), (-1,)):
        assert pool(src=(0,), op=op) == -1 and b"unknown op" in lib.sn_last_error()
    assert pool(flags=2) == -1 and b"flags" in lib.sn_last_error()
    # a MEAN plane's range: finite, hi > lo; not looked at for a column no MEAN plane reads
    for bad in ((1.0, 1.0), (2.0, 1.0), (float("nan"), 1.0), (0.0, float("inf")), (float("-inf"), 0.0)):
        assert pool(src=(3,), op=(0,), ranges=bad + (0.0, 1.0)) == -1 and b"value range" in lib.sn_last_error()
        assert pool(src=(4,), op=(0,), ranges=(0.0, 1.0) + bad) == -1 and b"value range" in lib.sn_last_error()
    assert pool(src=(3,), op=(0,), ranges=None) == -1 and b"value_range is null" in lib.sn_last_error()
    for kw in (dict(total=0), dict(total=-5), dict(B=0), dict(B=-1)):
        assert pool(**kw) == -1 and b"positive" in lib.sn_last_error()
    for dims in ((0, 4, 4), (4, -1, 4), (4, 4, 0)):
        assert pool(dims=dims) == -1 and b"extent" in lib.sn_last_error()
    assert pool(total=1 << 31) == -2 and b"2^31" in lib.sn_last_error()
    assert pool(B=65537) == -2 and b"B=65537" in lib.sn_last_error()
    assert pool(dims=(2048, 2048, 512)) == -2 and b"2^31" in lib.sn_last_error()
    assert pool(dims=(9000, 1, 1)) == -2 and b"LDS" in lib.sn_last_error()
    # the call accumulates in its outputs: no workspace for any shape, and `ws` is not looked at
    for shape in ((2, 4, 4, 4, 3), (32, 64, 64, 64, 8), (0, 4, 4, 4, 3)):
        assert lib.sn_voxel_pool_ws_bytes(*shape) == 0 == _hip.voxel_pool_ws_bytes(shape[0], shape[1:4], shape[4])
    assert pool(ws=off(4), total=0) == -1 and b"positive" in lib.sn_last_error()
    assert lib.sn_voxel_pool_chunk_points() == _hip.voxel_pool_chunk_points() == 1024


def test_layers_refuse_cpu_tensors_and_bad_planes():
    import torch
    from scene_net_amd.voxel_pool import parse_planes
    assert parse_planes(("x.mean", "v1.max", "z.min", "z.mean"), 2) == ([0, 4, 2, 2], [0, 2, 1, 0])
    for bad, C in ((("w.mean",), 0), (("x.sum",), 0), (("v0.mean",), 0), (("v2.max",), 2), ((), 0), (("x.min",) * 9, 0)):
        with pytest.raises(ValueError):
            parse_planes(bad, C)
    batch = sna.PointBatch(torch.zeros((4, 3), dtype=torch.float64), None, torch.tensor([0, 4]), (4,))
    with pytest.raises(sna.HipLibraryError):
        sna.voxel_pool(batch)
    for name in ("VoxelPool", "voxel_pool", "voxel_centroids", "centroid_hist_on_voxel", "centroid_reg_on_voxel",
                 "voxel_downsample", "xyz_Voxelization", "xyz_ToFullDense"):
        assert hasattr(sna, name) and name in sna.__all__
    x = torch.tensor([[0.0, 2.0]], dtype=torch.float64)
    xyz, dense, lab = sna.xyz_ToFullDense()((x, x, x))
    assert xyz is x and torch.equal(dense, torch.tensor([[0.0, 1.0]], dtype=torch.float64)) and torch.equal(lab, dense)


@pytest.mark.parametrize("kind,dims", KINDS)
def test_restatement_stays_inside_twice_the_derived_bound(kind, dims):
    """Half a quantum per row is span * 2^-33; the restatement is held to span * 2^-32 + 4 ulp(max(|lo|, |hi|))."""
    desc, own, tiles = pc.foreign_case(kind, dims)
    planes, counts, unbinned, nan_rows = pc.expected_pool(desc, dims, tiles, *pc.CENTROIDS, own=None)
    nx, ny, nz = dims
    worst = 0.0
    for b, t in enumerate(tiles):
        lo, hi = desc[b, :3], desc[b, 3:6]
        for a in range(3):      # no quantum leaves [0, 2^32]
            q = pc.quanta(t[~np.isnan(t[:, a]), a], lo[a], hi[a])
            assert q.min(initial=0) >= 0 and q.max(initial=0) <= 2 ** 32
        assert counts[b].sum() + unbinned[b] + nan_rows[b] == len(t) and nan_rows[b] == 0
        cells, means = pc.fsum_means(desc[b], dims, t)
        assert np.array_equal(np.flatnonzero(counts[b].reshape(-1)), cells)
        got = planes[b].reshape(3, -1)[:, cells].T
        bound = (hi - lo) * 2.0 ** -32 + 4 * np.spacing(np.maximum(np.abs(lo), np.abs(hi)))
        err = np.abs(got - means)
        assert (err <= bound).all(), (b, (err / bound).max())
        worst = max(worst, float((err / bound).max(initial=0.0)))
        assert (planes[b].reshape(3, -1)[:, counts[b].reshape(-1) == 0] == 0.0).all()
    assert counts[3].sum() == 0 and unbinned[3] == len(tiles[3])          # the tile with nothing binned
    # (a padded table takes what lies above a tile's own last edge into its cell n_a: few rows are outside it)
    assert counts[0].sum() > 500 and unbinned[:3].sum() > (100 if kind != "sized" else 0) and 0.0 < worst <= 1.0


def test_restatement_does_not_depend_on_the_order_of_the_rows():
    dims = (8, 12, 4)
    desc, own, tiles = pc.foreign_case("own", dims)
    rng = np.random.default_rng(240)
    values = [pc.special_values(len(t), rng)[:, None] for t in tiles]
    first = pc.expected_pool(desc, dims, tiles, *pc.EIGHT, values=values, ranges=[pc.VALUE_RANGE], fill=-1.0)
    assert first[3].sum() > 50 and np.isinf(first[0]).any()
    for seed in (1, 2):
        order = [np.random.default_rng(seed + b).permutation(len(t)) for b, t in enumerate(tiles)]
        again = pc.expected_pool(desc, dims, [t[o] for t, o in zip(tiles, order)], *pc.EIGHT,
                                 values=[v[o] for v, o in zip(values, order)], ranges=[pc.VALUE_RANGE], fill=-1.0)
        assert np.array_equal(pc.bits(first[0]), pc.bits(again[0]))
        assert all(np.array_equal(a, b) for a, b in zip(first[1:], again[1:]))
    for b, t in enumerate(tiles):
        assert first[1][b].sum() + first[2][b] + first[3][b] == len(t)
    # the mean of a plane lies between its minimum and maximum, up to one quantum; -0.0 and +0.0 keep their signs
    mean, low, high = first[0][:, 3], first[0][:, 4], first[0][:, 5]
    hit = first[1] > 0
    quantum = (pc.VALUE_RANGE[1] - pc.VALUE_RANGE[0]) * 2.0 ** -32
    clamp = lambda x: np.clip(x, *pc.VALUE_RANGE)   # noqa: E731
    assert (mean[hit] >= clamp(low[hit]) - quantum).all() and (mean[hit] <= clamp(high[hit]) + quantum).all()
    # of -0.0 and +0.0 in one voxel MIN gives -0.0 and MAX +0.0
    tile = pc.cube_tile(50, 6)
    d = pc.own_desc(tile, dims)[None]
    z = np.array([[0.0], [-0.0], [0.0]])
    got = pc.expected_pool(d, dims, [tile[:1].repeat(3, 0)], [3, 3], [pc.MIN, pc.MAX], values=[z])[0].reshape(2, -1)
    f = bc.expected_flat(d[0], dims, tile[:1])[0]
    assert got[0, f] == 0 and np.signbit(got[0, f]) and got[1, f] == 0 and not np.signbit(got[1, f])


def test_a_one_point_tile_gives_lo():
    dims = (5, 7, 3)
    pt = pc.cube_tile(1, 77)
    desc = pc.own_desc(pt, dims)[None]
    assert np.array_equal(desc[0, :3], desc[0, 3:6]) and np.array_equal(desc[0, :3], pt[0])
    # -inf is clipped into bin 0 and counts as lo: (-inf - lo) * 0 is NaN, which the clamp takes as 0
    for tile in (pt, np.concatenate([pt, [[-np.inf, pt[0, 1], pt[0, 2]]]])):
        planes, counts, unbinned, _ = pc.expected_pool(desc, dims, [tile], *pc.CENTROIDS, fill=np.nan)
        assert counts.sum() == len(tile) and unbinned[0] == 0 and counts.reshape(-1)[0] == len(tile)
        assert np.array_equal(pc.bits(planes.reshape(3, -1)[:, 0]), pc.bits(pt[0]))
        assert np.isnan(planes.reshape(3, -1)[:, 1:]).all()
