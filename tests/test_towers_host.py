"""Tower proposals, the part that needs no GPU: the stencil the C entry builds, its argument checks, the workspace size,
the numpy oracle of the definition against sklearn's DBSCAN, and the host mirrors of filter_towers / aggregate_centroids."""
import ctypes

import numpy as np
import pytest

import scene_net_amd as sna
from scene_net_amd import _hip

import towers_cases as tc

STENCILS = (   # eps, voxel_size, offsets (measured with the formula of the definition)
    (3.5, None, 179),
    (3.0, None, 123),
    (1.6, (1.3, 0.5, 0.5), 55),
    (7.0, None, 1419),
    (10.0, None, 4169),
)


@pytest.mark.parametrize("eps,voxel_size,count", STENCILS)
def test_stencil_equals_the_oracle_offsets(eps, voxel_size, count):
    rows, n = _hip.towers_stencil(eps, voxel_size)
    want = tc.stencil_offsets(eps, voxel_size)
    assert len(want) == count
    assert n == count
    assert tc.rows_to_offsets(rows.tolist()) == want
    pairs = [(r[0], r[1]) for r in rows.tolist()]
    assert pairs == sorted(set(pairs)), "rows ascend in (d0, d1), one per pair"


def test_stencil_tie_and_radius_limit():
    offs = set(tc.rows_to_offsets(_hip.towers_stencil(3.0)[0].tolist()))
    assert {(3, 0, 0), (0, -3, 0), (0, 0, 3), (2, 2, 1), (-1, 2, 2)} <= offs, "r^2 = 9 is inside at eps 3"
    assert (2, 2, 2) not in offs and (3, 1, 0) not in offs
    lib = _hip.load()
    n = ctypes.c_int64(-7)
    np_ = ctypes.cast(ctypes.pointer(n), ctypes.c_void_p)
    want = tc.stencil_offsets(10.999)                                       # 10 voxels along every axis: still served
    assert lib.sn_towers_stencil(10.999, None, None, 0, np_) == len({(a, b) for a, b, _ in want}) and n.value == len(want)
    assert lib.sn_towers_stencil(11.0, None, None, 0, None) == -2
    assert b"10 voxels" in lib.sn_last_error()
    size = (ctypes.c_double * 3)(1.0, 1.0, 0.25)
    assert lib.sn_towers_stencil(3.5, ctypes.cast(size, ctypes.c_void_p), None, 0, None) == -2   # 14 voxels along axis 2
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert lib.sn_towers_stencil(bad, None, None, 0, None) == -1
    size = (ctypes.c_double * 3)(1.0, 0.0, 1.0)
    assert lib.sn_towers_stencil(3.5, ctypes.cast(size, ctypes.c_void_p), None, 0, None) == -1
    # a short row buffer is filled as far as it goes and the full count still comes back
    rows = (ctypes.c_int32 * 6)(*([99] * 6))
    assert lib.sn_towers_stencil(3.5, None, ctypes.cast(rows, ctypes.c_void_p), 1, None) == 37
    assert list(rows) == [-3, -1, 1, 99, 99, 99]


def test_argument_checks_need_no_gpu():
    lib = _hip.load()
    buf = ctypes.create_string_buffer(256)
    p = ctypes.cast(buf, ctypes.c_void_p)
    big = ctypes.c_size_t(1 << 40)

    def call(grid=p, dtype=_hip.SN_F32, B=1, n=(8, 8, 8), tau=0.65, eps=3.5, size=None, min_points=18, max_towers=4,
             ws=p, ws_bytes=big, labels=p, n_towers=p, stats=p):
        return lib.sn_tower_proposals(grid, dtype, B, n[0], n[1], n[2], tau, eps, size, min_points, max_towers, ws,
                                      ws_bytes, labels, n_towers, stats, None)

    for name in ("grid", "ws", "labels", "n_towers", "stats"):
        assert call(**{name: None}) == -1, name
        assert b"null" in lib.sn_last_error() or name == "stats"
    assert call(stats=None, max_towers=0, ws_bytes=ctypes.c_size_t(0)) == -1   # (legal so far: fails on the workspace)
    assert b"sn_towers_ws_bytes" in lib.sn_last_error()
    assert call(B=0) == -1 and call(B=-3) == -1
    assert call(n=(8, 0, 8)) == -1
    assert call(min_points=0) == -1
    assert call(max_towers=-1) == -1
    for eps in (0.0, -2.0, float("nan"), float("inf")):
        assert call(eps=eps) == -1, eps
    assert call(eps=11.0) == -2
    for tau in (0.0, 1.0, -0.1, 1.5, float("nan")):
        for dt in (_hip.SN_F32, _hip.SN_BF16, _hip.SN_F64):
            assert call(tau=tau, dtype=dt) == -1, (tau, dt)
    assert b"tau" in lib.sn_last_error()
    need = lib.sn_towers_ws_bytes(1, 8, 8, 8)
    assert need > 0
    assert call(ws_bytes=ctypes.c_size_t(need - 1)) == -1
    assert b"sn_towers_ws_bytes" in lib.sn_last_error()
    # uint8 / bool grids ignore tau: the same call gets past the tau check and fails on the short workspace instead
    assert call(tau=7.0, dtype=_hip.SN_U8, ws_bytes=ctypes.c_size_t(need - 1)) == -1
    assert b"sn_towers_ws_bytes" in lib.sn_last_error()
    assert call(dtype=_hip.SN_I32) == -2       # a dtype of the library that is no grid dtype
    assert call(dtype=17) == -1
    assert call(n=(4096, 4096, 64)) == -2      # beyond 2^24 voxels per tile
    assert call(grid=ctypes.c_void_p(p.value + 2)) == -1                     # fp32 grid off its element alignment
    assert call(labels=ctypes.c_void_p(p.value + 2)) == -1
    assert lib.sn_tower_proposals_launches(p, 0, 1, 8, 8, 8, 0.65, 3.5, None, 18, 4, p, big, p, p, p, 0, 6, None) == -1
    assert lib.sn_tower_proposals_launches(p, 0, 1, 8, 8, 8, 0.65, 3.5, None, 18, 4, p, big, p, p, p, 3, 2, None) == -1


def test_ws_bytes():
    lib = _hip.load()
    for shape in ((0, 8, 8, 8), (1, 0, 8, 8), (1, 8, -1, 8), (1, 8, 8, 0), (1, 4096, 4096, 64), (1 << 20, 128, 128, 128)):
        assert lib.sn_towers_ws_bytes(*shape) == 0, shape
    assert lib.sn_towers_ws_bytes(65535, 4, 4, 4) > 0 and lib.sn_towers_ws_bytes(65536, 4, 4, 4) == 0, "at most 65535 tiles"
    sizes = [lib.sn_towers_ws_bytes(B, 64, 64, 64) for B in range(1, 40)]
    assert all(a > 0 for a in sizes) and all(b > a for a, b in zip(sizes, sizes[1:])), "monotone in B"
    assert lib.sn_towers_ws_bytes(1, 128, 128, 128) > 0, "128^3 per tile is served"
    assert lib.sn_towers_ws_bytes(1, 6, 5, 70) == lib.sn_towers_ws_bytes(1, 6, 5, 128), "rows are padded to whole words"
    for shape in ((1, 13, 13, 130), (3, 5, 7, 9), (1, 1, 1, 1)):
        assert lib.sn_towers_ws_bytes(*shape) % 8 == 0, "a whole number of 8-byte words, also for an odd word count"
    with pytest.raises(_hip.HipLibraryError):
        _hip.towers_ws_bytes(1, 4096, 4096, 64)


def test_cpu_tensors_raise():
    import torch
    with pytest.raises(sna.HipLibraryError, match="no CPU path"):
        sna.tower_proposals(torch.zeros(1, 4, 4, 4), tau=0.5)


@pytest.mark.parametrize("shape,density,eps,min_points,voxel_size", tc.SKLEARN_CASES)
def test_oracle_against_sklearn(shape, density, eps, min_points, voxel_size):
    cluster = pytest.importorskip("sklearn.cluster")
    grid = tc.random_grid(shape, density)
    s = np.array((1.0, 1.0, 1.0) if voxel_size is None else voxel_size)
    if voxel_size is not None:
        # about the inputs: no offset sits on the boundary, where sklearn's sqrt form and the squared form could disagree
        r = [int(eps / v) + 2 for v in s]
        d = np.stack(np.meshgrid(*[np.arange(-k, k + 1) for k in r], indexing="ij"), -1).reshape(-1, 3) * s
        d2 = (d * d).sum(axis=1)
        assert np.all(np.abs(d2 - eps * eps) > 1e-9 * eps * eps)
    labels, K, _, core = tc.dbscan_grid(grid, eps, min_points, voxel_size)
    idx = np.argwhere(grid)
    model = cluster.DBSCAN(eps=eps, min_samples=min_points).fit(idx * s)
    sk = np.full(shape, -2, dtype=np.int64)
    sk[grid] = model.labels_
    sk_core = np.zeros(shape, dtype=bool)
    sk_core[tuple(idx[model.core_sample_indices_].T)] = True
    assert np.array_equal(core, sk_core), "core set"
    assert np.array_equal((labels == -1) & grid, sk == -1), "noise set"
    assert np.all(labels[~grid] == -1)
    # the partition of the cores: ours -> sklearn's is a bijection
    ours, theirs = labels[core], sk[core]
    pairs = set(zip(ours.tolist(), theirs.tolist()))
    assert len(pairs) == K == len(set(ours.tolist())) == len(set(theirs.tolist()))
    # every border voxel belongs to a cluster that has a core within eps of it
    border = grid & ~core & (labels >= 0)
    assert np.array_equal(border, grid & ~core & (sk >= 0))
    cores = np.argwhere(core)
    for v in np.argwhere(border):
        near = (((cores - v) * s) ** 2).sum(axis=1) <= eps * eps
        assert labels[tuple(v)] in set(labels[tuple(cores[near].T)].tolist())
    assert K > 0 and border.any() or shape == (16, 16, 16), "the case exercises clusters and borders"


def test_filter_towers_and_aggregate_centroids_mirror_the_reference():
    # a hand-made table in xyz columns (height last), as the reference's code assumes ...
    rng = np.random.default_rng(3)
    def blob(center, extent, n=40):
        return np.asarray(center) + (rng.random((n, 3)) - 0.5) * np.asarray(extent)
    towers_xyz = [blob((10.0, 11.0, 8.0), (2.0, 2.0, 16.0)),    # tall: kept whatever its footprint
                  blob((12.0, 9.0, 3.0), (9.0, 1.0, 4.0)),      # a wall: low and wide
                  blob((7.0, 8.0, 2.0), (1.5, 1.5, 3.0)),       # low and compact: kept
                  blob((24.0, 10.0, 2.0), (1.5, 1.5, 3.0)),     # compact but at the rim of the cut-out
                  blob((10.5, 11.2, 4.0), (1.0, 1.0, 2.0))]     # close to the first in the plane
    cents_xyz = np.stack([t.mean(axis=0) for t in towers_xyz])
    center_xyz = np.array([10.0, 10.0, 5.0])
    threshold = 2.5

    # ... and the literal restatement of utils/observer_utils.py:476-549 on it
    def ref_filter(towers, centroids, threshold, xyz_center):
        keep = np.zeros(len(towers), dtype=bool)
        tower_height, radius = 14, 15
        for i, t in enumerate(towers):
            t_min, t_max = np.min(t, axis=0), np.max(t, axis=0)
            xy_var = np.max(t_max[:-1] - t_min[:-1])
            t_height = t_max[-1] - t_min[-1]
            if t_height >= tower_height:
                keep[i] = True
            else:
                keep[i] = xy_var <= threshold
            keep[i] = keep[i] and np.sum((centroids[i][:-1] - xyz_center[:-1]) ** 2) <= (radius - threshold * 2) ** 2
        return [towers[i] for i in range(len(towers)) if keep[i]], centroids[keep]

    def ref_aggregate(vxg_centroids):
        filtered = None
        min_euc = 1.5
        if len(vxg_centroids) == 0:
            return np.empty((0, 2))
        vxg_centroids = vxg_centroids[:, :-1]
        for vxg_c in vxg_centroids:
            c_full = np.full_like(vxg_centroids, vxg_c)
            euc = np.linalg.norm(c_full - vxg_centroids, axis=1)
            new_point = np.mean(vxg_centroids[euc <= min_euc], axis=0)
            filtered = [new_point] if filtered is None else np.concatenate((filtered, [new_point]))
        return np.unique(filtered, axis=0)

    want_t, want_c = ref_filter(towers_xyz, cents_xyz, threshold, center_xyz)
    assert [len(want_t), len(towers_xyz)] == [3, 5], "the table exercises every rule"
    got_t, got_c = sna.filter_towers(towers_xyz, cents_xyz, threshold, center_xyz, height_axis=2)
    assert len(got_t) == len(want_t) and all(np.array_equal(a, b) for a, b in zip(got_t, want_t))
    assert np.array_equal(got_c, want_c)
    want_a = ref_aggregate(cents_xyz)
    assert want_a.shape == (4, 2), "two centroids merge"
    assert np.array_equal(sna.aggregate_centroids(cents_xyz, height_axis=2), want_a)
    assert sna.aggregate_centroids(np.empty((0, 3))).shape == (0, 2)

    # the default height axis is grid axis 0 ([nz, nx, ny] grids): the same table with the height moved to the front
    zxy = [2, 0, 1]
    got_t, got_c = sna.filter_towers([t[:, zxy] for t in towers_xyz], cents_xyz[:, zxy], threshold, center_xyz[zxy])
    assert all(np.array_equal(a[:, [1, 2, 0]], b) for a, b in zip(got_t, want_t)) and len(got_t) == len(want_t)
    assert np.array_equal(got_c[:, [1, 2, 0]], want_c)
    assert np.array_equal(sna.aggregate_centroids(cents_xyz[:, zxy]), want_a)
