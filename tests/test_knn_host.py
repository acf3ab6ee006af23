"""Nearest neighbours (K21), the part that needs no GPU: the numpy oracle against sklearn's kd-tree, the host restatement
of avg_dist_points against the reference's recorded values, and the argument checks of the C entries."""
import ctypes
import os

import numpy as np
import pytest
import torch

import scene_net_amd as sna
from scene_net_amd import _hip

import knn_cases as kc


@pytest.mark.parametrize("which", range(4))
def test_oracle_equals_sklearn_on_blobs(which):
    from sklearn.neighbors import NearestNeighbors
    P, r, k = kc.blobs_case(which)[0], kc.BLOB_RADIUS[which], 8
    d2, found, mean, index = kc.oracle_of_blobs(which, k)
    full = found >= k
    assert full.sum() > 500 and (found == 0).sum() > 20 and ((found > 0) & ~full).sum() > 50, "full, partial and empty lists"
    dist, ind = NearestNeighbors(n_neighbors=k + 1, algorithm="kd_tree").fit(P).kneighbors(P)
    assert np.array_equal(ind[:, 0], np.arange(len(P))), "a point is its own nearest (no duplicates in these sets)"
    assert np.array_equal(ind[full, 1:], index[full])
    assert np.array_equal(dist[full, 1:], np.sqrt(d2[full]))
    # the columns are consistent with each other
    with np.errstate(invalid="ignore"):
        assert np.all(np.diff(d2, axis=1)[np.isfinite(d2[:, 1:])] >= 0) and np.all(np.isinf(d2[found == 0]))
    assert np.array_equal(np.isfinite(d2).sum(axis=1), np.minimum(found, k)) and np.array_equal(index < 0, np.isinf(d2))
    assert np.all(np.isnan(mean[found == 0])) and not np.isnan(mean[found > 0]).any()


def test_blob_case_of_the_issue():
    d2, found, mean, index = kc.oracle_of_blobs(2, 8)
    assert len(found) == 1900 and 0.70 < (found >= 8).mean() < 0.82 and 0.05 < (found == 0).mean() < 0.15


def test_oracle_breaks_ties_by_row_index():
    P, _, _ = kc.rim_case(0)
    d2, found, mean, index = kc.knn_oracle(P, 5.0, 16)
    ties = (np.diff(d2, axis=1) == 0) & np.isfinite(d2[:, 1:])
    assert ties.sum() > 1000, "an integer lattice: many equal distances"
    assert np.all(np.diff(index, axis=1)[ties] > 0), "equal distances in ascending row order"
    perm = np.random.default_rng(2).permutation(len(P))
    d2p, foundp, meanp, indexp = kc.knn_oracle(P[perm], 5.0, 16)
    assert np.array_equal(d2p, d2[perm]) and np.array_equal(foundp, found[perm])
    assert np.array_equal(meanp, mean[perm], equal_nan=True)


def test_exclude_zero_drops_duplicates():
    P = np.array([[1.0, 2.0, 3.0], [1.0, 2.0, 3.0], [1.0, 2.0, 4.0]]) + kc.ORIGIN
    d2, found, mean, index = kc.knn_oracle(P, 2.0, 2)
    assert found.tolist() == [2, 2, 2] and d2[0].tolist() == [0.0, 1.0] and index[0].tolist() == [1, 2] and mean[0] == 0.5
    d2, found, mean, index = kc.knn_oracle(P, 2.0, 2, exclude_zero=True)
    assert found.tolist() == [1, 1, 2] and d2[0].tolist() == [1.0, np.inf] and index[0].tolist() == [2, -1]
    assert index[2].tolist() == [0, 1], "two equal distances: the smaller row first"


def test_avg_dist_points_restated_against_the_reference(golden_dir):
    g = np.load(os.path.join(golden_dir, "avg_dist_points.npz"))
    names = [str(n) for n in g["names"]]
    clouds = {name: (xyz, acc, nd) for name, xyz, acc, nd in kc.golden_clouds()}
    assert names == list(clouds) and len(names) == 6
    seen_nd, seen_acc = set(), set()
    for name in names:
        xyz, (acc, nd), want = g[name + "_xyz"], g[name + "_args"], float(g[name + "_value"])
        assert np.array_equal(xyz, clouds[name][0]) and (acc, nd) == clouds[name][1:], "the committed clouds are the cases'"
        assert 25 <= len(xyz) <= 80 and xyz.min() > 100.0, "small clouds at UTM offsets"
        nd, m = int(nd), round(len(xyz) * acc)
        got = kc.avg_dist_points_host(xyz, acc, nd)
        print(f"{name}: reference {want!r} restatement {got!r} rel {abs(got - want) / abs(want):.2e}")
        assert abs(got - want) <= kc.avg_dist_bound(m, nd) * abs(want), name
        seen_nd.add(nd), seen_acc.add(float(acc))
    assert {1, 3, 5, 16} <= seen_nd and {1.0, 0.5} <= seen_acc
    dup = g["duplicate40_xyz"]
    assert len(np.unique(dup, axis=0)) == len(dup) - 1, "one duplicated point"
    short = g["short30_xyz"]
    assert round(len(short) * 0.1) * (round(len(short) * 0.1) - 1) < 16, "fewer positive distances than num_dists"


def test_running_means_is_the_reference_loop():
    """the literal loop of pcd_processing.py:477-505 over the oracle's distances against the merge of the per-row tables"""
    rng = np.random.default_rng(5)
    for m, nd in ((12, 3), (20, 16), (9, 1)):
        P = kc.ORIGIN + rng.random((m, 3)) * 4.0
        P[m // 2] = P[0]
        D = np.sqrt(kc.squared_distances(P))
        dists, avgs = [], []
        for i in range(m):
            dists += [d for d in D[i] if d > 0]
            avgs.append(np.mean(np.sort(dists)[:nd]))
        assert kc.avg_dist_points_host(P, 1.0, nd) == float(np.mean(avgs))


def test_chunk_points_and_ws_bytes():
    lib = _hip.load()
    assert lib.sn_knn_chunk_points() == _hip.knn_chunk_points() == 256
    # 0 for what the entry refuses
    for total, B, cells in ((0, 1, 1), (-5, 1, 1), (1 << 31, 1, 1), (10, 0, 1), (10, -1, 1), (10, 1, 0), (10, 1, (1 << 22) + 1),
                            (10, 3, (1 << 22) // 3 + 1), (10, 1 << 23, 1)):
        assert lib.sn_knn_ws_bytes(total, B, cells) == 0, (total, B, cells)
    a, b = lib.sn_knn_ws_bytes(1000, 1, 10), lib.sn_knn_ws_bytes(2000, 1, 10)
    assert 0 < a < b and b - a <= 1000 * 36 + 5 * 40 + 64
    assert lib.sn_knn_ws_bytes(1000, 4, 10) > a and lib.sn_knn_ws_bytes(1000, 1, 100) - a == 90 * 8
    assert lib.sn_knn_ws_bytes((1 << 31) - 1, 1, 1 << 22) > 0 and lib.sn_knn_ws_bytes(10, 4, 1 << 20) > 0
    with pytest.raises(_hip.HipLibraryError):
        _hip.knn_ws_bytes(0, 1, 1)


def test_argument_checks_need_no_gpu():
    lib = _hip.load()
    buf = ctypes.create_string_buffer(512)
    base = (ctypes.addressof(buf) + 15) // 16 * 16
    p = ctypes.c_void_p(base)
    off = lambda d: ctypes.c_void_p(base + d)   # noqa: E731
    big = ctypes.c_size_t(1 << 40)

    def knn(pts=p, offsets=p, total=100, B=2, radius=2.0, k=8, flags=0, lo=p, dx=4, dy=4, dz=4, mult=1, ws=p, ws_bytes=big,
            d2=p, found=p, mean=p, index=p):
        return lib.sn_knn_points(pts, offsets, total, B, radius, k, flags, lo, dx, dy, dz, mult, ws, ws_bytes, d2, found, mean,
                                 index, None)

    def stats(mean=p, found=p, offsets=p, total=100, B=2, k=8, ws=p, ws_bytes=big, out=p):
        return lib.sn_knn_tile_stats(mean, found, offsets, total, B, k, ws, ws_bytes, out, None)

    for name in ("pts", "offsets", "lo", "ws", "d2", "found"):
        assert knn(**{name: None}) == -1, name
        assert b"null" in lib.sn_last_error()
    for kw, word in (({"total": 0}, b"total"), ({"total": -3}, b"total"), ({"B": 0}, b"B must"), ({"B": -1}, b"B must"),
                     ({"k": 0}, b"k must"), ({"k": -2}, b"k must"), ({"radius": 0.0}, b"radius"), ({"radius": -1.0}, b"radius"),
                     ({"radius": float("nan")}, b"radius"), ({"radius": float("inf")}, b"radius"), ({"dx": 0}, b"dims"),
                     ({"dy": -1}, b"dims"), ({"dz": 0}, b"dims"), ({"mult": 0}, b"mult"), ({"flags": 2}, b"flags")):
        assert knn(**kw) == -1, kw
        assert word in lib.sn_last_error(), (kw, lib.sn_last_error())
    for kw, word in (({"k": 17}, b"k beyond"), ({"total": 1 << 31}, b"2^31"), ({"dx": 1 << 11, "dy": 1 << 11, "dz": 2}, b"cells"),
                     ({"B": 3, "dx": 128, "dy": 128, "dz": 128}, b"cells"), ({"radius": 1e-160}, b"radius"),
                     ({"radius": 1e160}, b"radius")):
        assert knn(**kw) == -2, kw
        assert word in lib.sn_last_error(), (kw, lib.sn_last_error())
    for name, d in (("pts", 4), ("offsets", 4), ("lo", 4), ("ws", 8), ("d2", 4), ("found", 2), ("mean", 4), ("index", 4)):
        assert knn(**{name: off(d)}) == -1, name
        assert b"aligned" in lib.sn_last_error()
    need = lib.sn_knn_ws_bytes(100, 2, 64)
    assert need > 0 and knn(ws_bytes=ctypes.c_size_t(need - 1)) == -1
    assert b"sn_knn_ws_bytes" in lib.sn_last_error()
    args = (p, p, 100, 2, 2.0, 8, 0, p, 4, 4, 4, 1, p, big, p, p, p, p)
    assert lib.sn_knn_points_launches(*args, 0, 3, None) == -1 and lib.sn_knn_points_launches(*args, 2, 5, None) == -1
    assert lib.sn_knn_points_launches(*args, 3, 2, None) == -1 and b"first" in lib.sn_last_error()

    for name in ("mean", "found", "offsets", "ws", "out"):
        assert stats(**{name: None}) == -1, name
        assert b"null" in lib.sn_last_error()
    for kw in ({"total": 0}, {"B": 0}, {"k": 0}):
        assert stats(**kw) == -1, kw
    assert stats(k=17) == -2 and stats(total=1 << 31) == -2 and stats(B=65536) == -2
    for name, d in (("mean", 4), ("found", 2), ("offsets", 4), ("ws", 8), ("out", 4)):
        assert stats(**{name: off(d)}) == -1, name
        assert b"aligned" in lib.sn_last_error()
    assert stats(ws_bytes=ctypes.c_size_t(8)) == -1 and b"sn_knn_ws_bytes" in lib.sn_last_error()


def test_cpu_tensors_and_limits_raise():
    pts = torch.zeros(8, 3, dtype=torch.float64)
    for call in (lambda: sna.knn_distances(pts, 2, 1.0), lambda: sna.point_spacing(pts, 1, 1.0),
                 lambda: sna.k_distance_curve(pts, 2, 1.0), lambda: sna.remove_outliers(pts, 2, 1.0),
                 lambda: sna.avg_dist_points(pts, 1.0, 2)):
        with pytest.raises(sna.HipLibraryError, match="no CPU path"):
            call()
    with pytest.raises(ValueError, match="16"):
        sna.avg_dist_points(pts, 1.0, 17)
    for name in ("PointNeighbours", "knn_distances", "point_spacing", "k_distance_curve", "remove_outliers", "avg_dist_points"):
        assert hasattr(sna, name) and name in sna.__all__
