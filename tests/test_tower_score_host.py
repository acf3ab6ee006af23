"""K11 without a GPU: the oracle of tests/tower_score_cases.py on statistics rows equals the host mirrors on real voxel
lists, the two C entries refuse bad arguments before any launch, and the Python layer refuses CPU tensors."""
import ctypes
import math

import numpy as np
import pytest
import torch

import scene_net_amd as sna
from scene_net_amd import _hip

import tower_score_cases as sc
import towers_cases as tc

# shape, seed, eps, min_points, voxel_size, threshold, tower_height, radius, height_axis
REAL_CASES = (
    ((16, 16, 16), 1, 1.0, 1, None, 1.0, 3.0, 9.0, 0),
    ((12, 13, 17), 2, 1.5, 3, None, 1.5, 4.0, 10.0, 2),
    ((9, 20, 33), 3, 0.8, 2, (1.3, 0.5, 0.75), 1.0, 3.0, 9.0, 1),
)


def _voxel_lists(labels):
    """TowerProposals.towers' lists: per cluster the voxel indices [n, 3] fp64 in memory order"""
    idx = np.argwhere(labels >= 0)
    ids = labels[labels >= 0]
    return [idx[ids == k].astype(np.float64) for k in range(int(ids.max()) + 1)]


@pytest.mark.parametrize("case", REAL_CASES, ids=lambda c: "x".join(map(str, c[0])))
def test_oracle_on_stats_equals_the_mirrors_on_voxel_lists(case):
    shape, seed, eps, min_points, voxel_size, threshold, tower_height, radius, h = case
    g = np.random.default_rng(seed).random(shape) < 0.12
    g[1:9, 1:3, 2:4] = True
    labels, K, stats, _ = tc.dbscan_grid(g, eps, min_points, voxel_size)
    s = sc.size_of(voxel_size)
    center = (np.array(shape, dtype=np.float64) - 1.0) / 2.0 * s
    voxels = _voxel_lists(labels)
    assert len(voxels) == K and K >= 3
    towers = [t * s for t in voxels]
    cents = np.stack([t.mean(axis=0) for t in voxels]) * s
    n_towers = np.array([K], dtype=np.int32)
    # the coordinate rule: centroids and extents from the integer rows equal those of the voxel lists bit for bit
    present, c, lo, hi = sc.coordinates(stats, K, voxel_size)
    assert present.all() and sc.same_bits(c, cents)
    assert sc.same_bits(hi - lo, np.stack([t.max(axis=0) - t.min(axis=0) for t in towers]))
    if voxel_size is None:   # TowerProposals.towers(b)'s centroids are the plain means
        assert sc.same_bits(c, np.stack([t.mean(axis=0) for t in voxels]))
    # filter -> aggregate
    kept, kept_c = sna.filter_towers(towers, cents, threshold, center, height_axis=h, tower_height=tower_height, radius=radius)
    want = sna.aggregate_centroids(kept_c, height_axis=h, min_euc=1.5)
    got = sc.centroids_oracle(stats[None], n_towers, h, voxel_size, center, True, threshold, tower_height, radius, 1.5)
    assert 0 < len(kept) < K, "the case filters some clusters and keeps some"
    assert int(got["keep"].sum()) == len(kept) and got["n_agg"][0] == len(want)
    assert sc.same_bits(got["agg"][0, :len(want)], want)
    assert np.isnan(got["agg"][0, len(want):]).all()
    # no filter -> aggregate -> match against itself shifted: compute_euc_dists' chain
    free = sc.centroids_oracle(stats[None], n_towers, h, voxel_size, None, False)
    assert sc.same_bits(free["agg"][0, :free["n_agg"][0]], sna.aggregate_centroids(cents, height_axis=h, min_euc=1.5))
    m = sc.match_oracle(free["agg"], free["n_agg"], free["status"], stats[None], n_towers, h, voxel_size, hit_dist=0.5)
    assert m["totals"][2] == K and m["totals"][4] + m["totals"][5] == K and m["totals"][4] > 0
    assert (m["dist"][0] >= 0).all() and (m["match"][0] >= 0).all()


def test_totals_loop_of_the_oracle():
    # two proposals; gt rows: one on the first (hit), one nearest to the second but beyond hit_dist (miss, false proposal)
    agg = np.array([[[1.0, 1.0], [10.0, 10.0], [np.nan, np.nan]]])
    gt, gn = sc.table([[sc.at((0, 1, 1)), sc.at((0, 10, 14))]], 4)
    m = sc.match_oracle(agg, np.array([2], np.int32), np.array([0], np.int32), gt, gn, hit_dist=3.0)
    assert m["match"][0].tolist() == [0, 1, -1, -1] and m["dist"][0, :2].tolist() == [0.0, 4.0]
    assert dict(zip(sc.TOTAL_NAMES, m["totals"].tolist())) == dict(
        tiles=1, tiles_skipped=0, gt_towers=2, proposals=2, hits=1, misses=1, false_proposals=1, reserved=0)
    v = sna.tower_detection_values(m["totals"], 0.0)
    assert v["recall"] == 0.5 and v["precision"] == 0.5 and v["f1"] == 0.5 and v["mean_error"] == 0.0
    assert sna.tower_detection_values([0] * 8, 0.0)["f1"] == 0.0       # 0/0 -> 0


def test_argument_checks_need_no_gpu():
    lib = _hip.load()
    buf = ctypes.create_string_buffer(256)
    p = ctypes.cast(buf, ctypes.c_void_p)
    ctr = (ctypes.c_double * 3)(0.0, 0.0, 0.0)
    c = ctypes.cast(ctr, ctypes.c_void_p)

    def centroids(stats=p, B=1, K=4, h=0, vs=None, center=c, filt=1, min_euc=1.5, keep=p, planar=p):
        return lib.sn_tower_centroids(stats, p, B, K, h, vs, center, filt, 1.75, 14.0, 25.0, min_euc, keep, planar, p, p, p,
                                      None)

    assert centroids(stats=None) == -1 and b"null" in lib.sn_last_error()
    assert centroids(keep=None) == -1
    assert centroids(K=1025) == -2 and b"1024" in lib.sn_last_error()
    assert centroids(B=65536) == -2
    assert centroids(h=3) == -1 and b"height_axis" in lib.sn_last_error()
    assert centroids(B=0) == -1 and centroids(K=0) == -1
    assert centroids(center=None) == -1          # the filter needs a centre
    assert centroids(min_euc=0.0) == -1 and centroids(min_euc=math.inf) == -1 and centroids(min_euc=math.nan) == -1
    bad = (ctypes.c_double * 3)(1.0, 0.0, 1.0)
    assert centroids(vs=ctypes.cast(bad, ctypes.c_void_p)) == -1 and b"voxel_size" in lib.sn_last_error()
    assert centroids(planar=ctypes.c_void_p(p.value + 4)) == -1 and b"aligned" in lib.sn_last_error()

    def match(agg=p, Kp=4, Kg=4, B=1, h=0, vs=None, hit=3.5, dist=p, totals=p, dist_total=p):
        return lib.sn_tower_match(agg, p, p, Kp, p, p, Kg, B, h, vs, hit, p, dist, None, totals, dist_total, None)

    assert match(agg=None) == -1 and b"null" in lib.sn_last_error()
    assert match(Kp=1025) == -2 and match(Kg=1025) == -2 and match(B=65536) == -2
    assert match(h=3) == -1 and match(h=-1) == -1
    assert match(B=0) == -1 and match(Kp=0) == -1
    assert match(hit=0.0) == -1 and match(hit=math.nan) == -1
    assert match(totals=None) == -1 and match(dist_total=None) == -1 and b"together" in lib.sn_last_error()
    assert match(vs=ctypes.cast(bad, ctypes.c_void_p)) == -1
    assert match(dist=ctypes.c_void_p(p.value + 4)) == -1 and b"aligned" in lib.sn_last_error()


def test_python_layer_refuses_cpu_tensors():
    grid = torch.zeros((1, 8, 8, 8))
    with pytest.raises(sna.HipLibraryError):
        sna.get_tower_proposals(grid, 0.65)
    with pytest.raises(sna.HipLibraryError):
        sna.compute_euc_dists(grid, grid.bool(), 0.65)
    with pytest.raises(sna.HipLibraryError):
        sna.TowerDetectionMetrics(hit_dist=3.5).update(grid, grid.bool())
    props = sna.TowerProposals(torch.zeros((1, 8, 8, 8), dtype=torch.int32), torch.zeros(1, dtype=torch.int32),
                               torch.zeros((1, 4, 12), dtype=torch.int64), 4)
    with pytest.raises(sna.HipLibraryError):
        sna.tower_centroids(props, 1.75)
    m = sna.TowerDetectionMetrics()
    assert m.hit_dist == m.eps == 3.5 and m.threshold == 1.75 and "totals" not in m.state_dict()
    with pytest.raises(ValueError):
        sna.TowerDetectionMetrics(hit_dist=0.0)
