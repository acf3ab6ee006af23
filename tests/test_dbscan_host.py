"""Point DBSCAN (K10), the part that needs no GPU: the numpy oracle against sklearn's kd-tree DBSCAN, the case sets, the
cell grid of sn_dbscan_cell_grid, and the argument checks of the C entries."""
import ctypes
import os

import numpy as np
import pytest
import torch

import scene_net_amd as sna
from scene_net_amd import _hip

import dbscan_cases as dc


def _sklearn_labels(P, eps, min_points):
    from sklearn.cluster import DBSCAN
    return DBSCAN(eps=eps, min_samples=min_points, algorithm="kd_tree").fit(P).labels_


@pytest.mark.parametrize("which", range(4))
def test_oracle_equals_sklearn_on_blobs(which):
    P, eps, mp = dc.blobs_case(which)
    assert P.shape == (1900, 3) and (eps, mp) == dc.PAIRS[which]
    assert dc.rim_pairs(P, eps) == 0, "the reference is only pinned away from the rim"
    cluster, K, stats, core = dc.oracle_of_blobs(which)
    assert np.array_equal(_sklearn_labels(P, eps, mp), cluster)
    border = (cluster >= 0) & ~core
    assert K >= 1 and core.sum() > 50 and border.sum() > 100 and (cluster < 0).sum() > 100, "cores, borders and noise"
    assert stats[:, 0].sum() == (cluster >= 0).sum() and stats[:, 1].sum() == core.sum()
    assert np.all(np.diff(stats[:, 2]) > 0), "ids ascend with the smallest core position"


@pytest.mark.parametrize("eps,mp,K,cores,rim", [(10.0, 300, 1, 700, 0), (3.5, 18, 1, 776, 0), (1.0, 10, 6, 753, 1)])
def test_oracle_equals_sklearn_on_the_golden_towers(golden_dir, eps, mp, K, cores, rim):
    """(at 1.0 / 10 one pair of the tile's centimetre coordinates lies inside the rim band; the labels agree all the same)"""
    T = dc.golden_towers(np.load(os.path.join(golden_dir, "ts40k_sample575_full.npz"))["tile"])
    assert T.shape == (776, 3)
    assert dc.rim_pairs(T, eps) == rim
    cluster, k, stats, core = dc.dbscan_oracle(T, eps, mp)
    assert (k, int(core.sum())) == (K, cores)
    assert np.array_equal(_sklearn_labels(T, eps, mp), cluster)


def test_rim_sets_sit_on_the_rim():
    P, eps, mp = dc.rim_case(0)
    on = dc.exact_rim_pairs(P, eps)
    assert on > 1000
    d = P[:, None, :] - P[None, :, :]
    assert ((np.abs(d) == [3, 4, 0]).all(axis=2)).any() and ((np.abs(d) == [0, 3, 4]).all(axis=2)).any()
    for shift in (1, -1):
        Q = dc.rim_case(shift)[0]
        assert np.abs(Q - P).max() <= np.spacing(dc.ORIGIN[1]) and dc.exact_rim_pairs(Q, eps) < on
        assert not np.array_equal(dc.neighbours(Q, eps), dc.neighbours(P, eps)), "one ulp moves pairs off the rim"


def test_contraction_set_is_large_enough():
    P, eps, mp, pairs, verdict = dc.contraction_case()
    assert pairs >= 100 and len(P) == 2 * pairs
    N = dc.neighbours(P, eps)
    for i in range(pairs):
        d = P[2 * i + 1] - P[2 * i]
        plain = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2] <= eps * eps
        assert bool(N[2 * i, 2 * i + 1]) is bool(plain) is bool(verdict[i])
        assert any((s <= eps * eps) != plain for s in dc.contracted_sums(*d)), "a contracted sum decides the other way"
        assert N[2 * i].sum() == 1 + int(plain), "pairs are isolated"
    assert dc.dbscan_oracle(P, eps, mp)[1] == verdict.sum() and 0 < verdict.sum() < pairs


def test_constructions_hold_in_the_oracle():
    for order in ("ascending", "descending", "shuffled"):
        P, eps, mp = dc.chain_case(order)
        cluster, K, stats, core = dc.dbscan_oracle(P, eps, mp)
        assert K == 1 and core.sum() == 2998 and (cluster == 0).all() and stats[0].tolist()[:2] == [3000, 2998]
    for order in ("AXB", "BXA", "XBA", "XAB"):
        P, eps, mp, x = dc.shared_border_case(order)
        cluster, K, stats, core = dc.dbscan_oracle(P, eps, mp)
        assert K == 2 and not core[x] and core.sum() == 8 and cluster[x] == 0, "the smaller id wins"
    P, labels, keep, odd = dc.nonfinite_case()
    sel = dc.isin_positions(labels, keep)
    assert set(odd) <= set(sel) and not np.isnan(labels[sel]).any() and np.isnan(labels).any()
    cluster = dc.dbscan_oracle(P[sel], 1.2, 5)[0]
    assert (cluster[np.isin(sel, odd)] == -1).all() and (cluster >= 0).sum() > 100
    assert np.array_equal(dc.dbscan_oracle(np.array([[np.nan, 0, 0], [1e300, 0, 0]]), 1.0, 1)[0], [-1, 0]), \
        "a NaN point is not its own neighbour; a huge finite one is"


def test_cell_grid():
    lo = dc.SEAM_LO
    grid = _hip.dbscan_cell_grid
    dims, side = grid(dc.SEAM_BOUNDS, 2.0, 1 << 18)
    assert side == 2.0 * (1.0 + 2.0 ** -20) and dims == (40, 40, 40), "floor(80 / side) + 1 cells per axis"
    # the smallest k whose grid fits
    for max_cells in (64000, 63999, 1000, 27, 26, 8, 7, 1):
        dims, side = grid(dc.SEAM_BOUNDS, 2.0, max_cells)
        k = round(side / (2.0 * (1.0 + 2.0 ** -20)))
        assert side == k * 2.0 * (1.0 + 2.0 ** -20)
        assert dims == (int(80.0 // side) + 1,) * 3 and dims[0] ** 3 <= max_cells
        if k > 1:
            smaller = (k - 1) * 2.0 * (1.0 + 2.0 ** -20)
            assert (int(80.0 // smaller) + 1) ** 3 > max_cells, "k - 1 would not fit"
    assert grid(dc.SEAM_BOUNDS, 2.0, 64000)[0] == (40, 40, 40) and grid(dc.SEAM_BOUNDS, 2.0, 63999)[0] == (20, 20, 20)
    assert grid(dc.SEAM_BOUNDS, 2.0, 1)[0] == (1, 1, 1)
    # degenerate bounds: a point, a plane, an anisotropic box
    assert grid(list(lo) + list(lo), 10.0, 100)[0] == (1, 1, 1)
    assert grid([0, 0, 5, 100, 100, 5], 10.0, 1 << 18)[0] == (10, 10, 1)
    assert grid([0, 0, 0, 1e6, 10, 0], 10.0, 1 << 22)[0][1:] == (1, 1)
    lib = _hip.load()
    b = (ctypes.c_double * 6)(0, 0, 0, 1, 1, 1)
    bp = ctypes.cast(b, ctypes.c_void_p)
    assert lib.sn_dbscan_cell_grid(bp, 1.0, 10, None, None) == 0, "both outputs are optional"
    assert lib.sn_dbscan_cell_grid(None, 1.0, 10, None, None) == -1
    for eps in (0.0, -1.0, float("nan"), float("inf")):
        assert lib.sn_dbscan_cell_grid(bp, eps, 10, None, None) == -1, eps
    assert lib.sn_dbscan_cell_grid(bp, 1.0, 0, None, None) == -1
    assert lib.sn_dbscan_cell_grid(bp, 1e-200, 10, None, None) == -2 and lib.sn_dbscan_cell_grid(bp, 1e200, 10, None, None) == -2
    assert lib.sn_dbscan_cell_grid(bp, 1.0, (1 << 22) + 1, None, None) == -2
    for bad in ((0, 0, 0, -1, 1, 1), (0, 0, 0, 1, float("inf"), 1), (float("nan"), 0, 0, 1, 1, 1), (-1e308, 0, 0, 1e308, 1, 1)):
        bb = (ctypes.c_double * 6)(*bad)
        assert lib.sn_dbscan_cell_grid(ctypes.cast(bb, ctypes.c_void_p), 1.0, 10, None, None) == -1, bad
    with pytest.raises(_hip.HipLibraryError):
        grid([0, 0, 0, -1, 1, 1], 1.0, 10)


def test_seam_points_sit_on_the_seams():
    for max_cells in (1 << 18, 64):
        dims, side = _hip.dbscan_cell_grid(dc.SEAM_BOUNDS, dc.SEAM_EPS, max_cells)
        P, eps, mp = dc.seam_case(side)
        assert len(P) == 81 and dc.exact_rim_pairs(P, eps) >= 54, "b and c are exactly eps from a"
        assert (P >= dc.SEAM_BOUNDS[:3]).all() and (P <= dc.SEAM_BOUNDS[3:]).all()
        on = sum(int((P[:, a] == dc.SEAM_LO[a] + j * side).sum()) for a in range(3) for j in (1, 2, 3))
        assert on >= 9


def test_ws_bytes_and_chunk_points():
    lib = _hip.load()
    assert lib.sn_points_select_chunk_points() == _hip.points_select_chunk_points() == 1024
    assert lib.sn_dbscan_chunk_points() == _hip.dbscan_chunk_points() == 256
    for n in (0, -1, (1 << 33) + 1):
        assert lib.sn_points_select_ws_bytes(n) == 0
    for n, chunks in ((1, 1), (1024, 1), (1025, 2), (10 ** 7, 9766)):
        assert lib.sn_points_select_ws_bytes(n) == 56 * chunks
    for capacity, cells in ((0, 1), (-1, 1), (1 << 31, 1), (1, 0), (1, (1 << 22) + 1)):
        assert lib.sn_dbscan_ws_bytes(capacity, cells) == 0, (capacity, cells)
    a, b = lib.sn_dbscan_ws_bytes(1000, 10), lib.sn_dbscan_ws_bytes(2000, 10)
    assert 0 < a < b and b - a <= 1000 * 48 + 64 and lib.sn_dbscan_ws_bytes((1 << 31) - 1, 1 << 22) > 0
    with pytest.raises(_hip.HipLibraryError):
        _hip.dbscan_ws_bytes(0, 1)
    with pytest.raises(_hip.HipLibraryError):
        _hip.points_select_ws_bytes(0)


def test_argument_checks_need_no_gpu():
    lib = _hip.load()
    buf = ctypes.create_string_buffer(512)
    base = (ctypes.addressof(buf) + 15) // 16 * 16
    p = ctypes.c_void_p(base)
    off = lambda d: ctypes.c_void_p(base + d)   # noqa: E731
    big = ctypes.c_size_t(1 << 40)
    bounds = (ctypes.c_double * 6)(0, 0, 0, 50, 50, 50)
    bp = ctypes.cast(bounds, ctypes.c_void_p)

    def select(pts=p, labels=p, n=100, keep=p, n_keep=2, capacity=10, ws=p, ws_bytes=big, sel=p, n_sel=p, bbox=p):
        return lib.sn_points_select(pts, labels, n, keep, n_keep, capacity, ws, ws_bytes, sel, n_sel, bbox, None)

    def cluster(pts=p, n=100, sel=p, n_sel=p, capacity=10, b=bp, eps=2.0, min_points=3, max_cells=1000, max_clusters=4, ws=p,
                ws_bytes=big, cl=p, n_clusters=p, stats=p, status=p):
        return lib.sn_dbscan_points(pts, n, sel, n_sel, capacity, b, eps, min_points, max_cells, max_clusters, ws, ws_bytes,
                                    cl, n_clusters, stats, status, None)

    for name in ("pts", "ws", "n_sel", "bbox", "keep"):
        assert select(**{name: None}) == -1, name
        assert b"null" in lib.sn_last_error()
    assert select(sel=None) == -1 and b"sel is needed" in lib.sn_last_error()
    for kw in ({"n": 0}, {"n": -3}, {"n_keep": -1}, {"capacity": -1}):
        assert select(**kw) == -1, kw
    assert select(n=(1 << 33) + 1) == -2 and select(n_keep=65) == -2
    need = lib.sn_points_select_ws_bytes(100)
    assert select(ws_bytes=ctypes.c_size_t(need - 1)) == -1
    assert b"sn_points_select_ws_bytes" in lib.sn_last_error()
    for name in ("pts", "labels", "keep", "ws", "sel", "n_sel", "bbox"):
        assert select(**{name: off(4)}) == -1, name
        assert b"aligned" in lib.sn_last_error()

    for name in ("pts", "ws", "cl", "n_clusters", "status", "b", "stats", "n_sel"):
        assert cluster(**{name: None}) == -1, name
    for eps in (0.0, -2.0, float("nan"), float("inf")):
        assert cluster(eps=eps) == -1, eps
        assert b"eps" in lib.sn_last_error()
    for kw in ({"min_points": 0}, {"min_points": -4}, {"n": 0}, {"capacity": 0}, {"max_clusters": -1}, {"max_cells": 0}):
        assert cluster(**kw) == -1, kw
    assert cluster(capacity=1 << 31) == -2 and cluster(max_cells=(1 << 22) + 1) == -2 and cluster(eps=1e-160) == -2
    assert cluster(max_clusters=(1 << 20) + 1) == -2
    dims, _ = _hip.dbscan_cell_grid(list(bounds), 2.0, 1000)
    need = lib.sn_dbscan_ws_bytes(10, dims[0] * dims[1] * dims[2])
    assert need > 0 and cluster(ws_bytes=ctypes.c_size_t(need - 1)) == -1
    assert b"sn_dbscan_ws_bytes" in lib.sn_last_error()
    for name, d in (("pts", 4), ("sel", 4), ("n_sel", 4), ("ws", 8), ("cl", 2), ("n_clusters", 2), ("stats", 4), ("status", 2)):
        assert cluster(**{name: off(d)}) == -1, name
        assert b"aligned" in lib.sn_last_error()
    assert lib.sn_dbscan_points_launches(p, 100, p, p, 10, bp, 2.0, 3, 1000, 4, p, big, p, p, p, p, 0, 3, None) == -1
    assert lib.sn_dbscan_points_launches(p, 100, p, p, 10, bp, 2.0, 3, 1000, 4, p, big, p, p, p, p, 2, 9, None) == -1


def test_cpu_tensors_raise():
    pts, classes = torch.zeros(8, 3, dtype=torch.float64), torch.zeros(8)
    with pytest.raises(sna.HipLibraryError, match="no CPU path"):
        sna.cluster_points(pts, 2.0, 3)
    with pytest.raises(sna.HipLibraryError, match="no CPU path"):
        sna.select_object(pts, classes, [15])
    with pytest.raises(sna.HipLibraryError, match="no CPU path"):
        sna.extract_towers(pts)
    with pytest.raises(sna.HipLibraryError, match="no CPU path"):
        sna.crop_two_towers_samples(pts, classes)
    with pytest.raises(sna.HipLibraryError, match="no CPU path"):
        sna.crop_tower_samples(pts, classes)
