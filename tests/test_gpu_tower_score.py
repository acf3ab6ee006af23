"""sn_tower_centroids / sn_tower_match (K11) on the device against the oracle of tests/tower_score_cases.py, which calls the
host mirrors sna.filter_towers / sna.aggregate_centroids and restates compute_euc_dists' matching loop in numpy.  Every
comparison is bit for bit (keep, planar, agg, n_agg, status, match, dist, totals); dist_total is checked as the header
defines it: identical over runs, and within hits * 2^-53 * sum(dist) of math.fsum.  Most cases fabricate the statistics
rows directly: the kernels read nothing else."""
import math
import os

import numpy as np
import pytest
import torch

import scene_net_amd as sna
from scene_net_amd import _hip

import tower_score_cases as sc
import towers_cases as tc

pytestmark = pytest.mark.gpu

ULP1 = float(np.nextafter(1.0, 2.0))


def _garbage(shape, dtype, dev):
    """an output buffer the kernel has to overwrite everywhere (every byte 0x55)"""
    nbytes = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    return torch.full((nbytes,), 0x55, dtype=torch.uint8, device=dev).view(dtype).reshape(shape)


def run_centroids(dev, stats, n_towers, height_axis=0, voxel_size=None, center=None, apply_filter=True, threshold=1.75,
                  tower_height=14.0, radius=15.0, min_euc=1.5):
    B, K = stats.shape[:2]
    st, nt = torch.from_numpy(stats).to(dev), torch.from_numpy(n_towers).to(dev)
    keep = _garbage((B, K), torch.uint8, dev)
    planar, agg = _garbage((B, K, 2), torch.float64, dev), _garbage((B, K, 2), torch.float64, dev)
    n_agg, status = _garbage((B,), torch.int32, dev), _garbage((B,), torch.int32, dev)
    rim_sq = (float(radius) - float(threshold) * 2) ** 2
    _hip.tower_centroids(st, nt, height_axis, None if center is None else [float(v) for v in center], apply_filter,
                         float(threshold), float(tower_height), rim_sq, float(min_euc), keep, planar, agg, n_agg, status,
                         voxel_size=voxel_size)
    return {k: v.cpu().numpy() for k, v in dict(keep=keep, planar=planar, agg=agg, n_agg=n_agg, status=status).items()}


def check_centroids(dev, stats, n_towers, what="", **kw):
    got = run_centroids(dev, stats, n_towers, **kw)
    want = sc.centroids_oracle(stats, n_towers, **kw)
    for name in ("keep", "planar", "agg", "n_agg", "status"):
        assert sc.same_bits(got[name], want[name]), f"{name} {what}"
    return got


def run_match(dev, agg, n_agg, status, gt_stats, gt_n_towers, height_axis=0, voxel_size=None, hit_dist=math.inf,
              totals=None, dist_total=None):
    B, Kg = gt_stats.shape[:2]
    match, dist = _garbage((B, Kg), torch.int32, dev), _garbage((B, Kg), torch.float64, dev)
    gt_planar = _garbage((B, Kg, 2), torch.float64, dev)
    _hip.tower_match(torch.from_numpy(np.ascontiguousarray(agg)).to(dev), torch.from_numpy(n_agg).to(dev),
                     torch.from_numpy(status).to(dev), torch.from_numpy(gt_stats).to(dev),
                     torch.from_numpy(gt_n_towers).to(dev), height_axis, hit_dist, match, dist, gt_planar, totals, dist_total,
                     voxel_size=voxel_size)
    return dict(match=match.cpu().numpy(), dist=dist.cpu().numpy(), gt_planar=gt_planar.cpu().numpy())


def check_match(dev, agg, n_agg, status, gt_stats, gt_n_towers, what="", **kw):
    """one call with fresh totals against the oracle; returns (got, want)"""
    totals = torch.zeros(sc.NTOTAL, dtype=torch.int64, device=dev)
    dist_total = torch.zeros(1, dtype=torch.float64, device=dev)
    got = run_match(dev, agg, n_agg, status, gt_stats, gt_n_towers, totals=totals, dist_total=dist_total, **kw)
    want = sc.match_oracle(agg, n_agg, status, gt_stats, gt_n_towers, **kw)
    for name in ("match", "dist", "gt_planar"):
        assert sc.same_bits(got[name], want[name]), f"{name} {what}"
    assert np.array_equal(totals.cpu().numpy(), want["totals"]), f"totals {what}"
    ref, bound = sc.dist_total_bound(want["hit_dists"])
    assert abs(float(dist_total.item()) - ref) <= bound, f"dist_total {what}"
    got["totals"], got["dist_total"] = totals.cpu().numpy(), float(dist_total.item())
    return got, want


# --------------------------------------------------------------------------- row counts
@pytest.mark.parametrize("K", (1, 2, 63, 64, 65, 130, 1024))
def test_row_counts(hip_device, K):
    extent = max(3, int(math.sqrt(K) * 2))
    # n_towers = K, 0 (an empty middle tile) and K + 3 (rows missing: status bit 0)
    stats, n_towers = sc.table([sc.random_rows(K, 10 + K, holes=min(2, K // 4)), [], sc.random_rows(K + 3, 20 + K)], K,
                               n_towers=[K, 0, K + 3])
    center = [extent / 2.0] * 3
    kw = dict(center=center, threshold=4.0, tower_height=9.0, radius=extent / 2.0 + 8.0)
    got = check_centroids(hip_device, stats, n_towers, f"K={K} filtered", **kw)
    assert got["status"].tolist() == [0, 0, 1] and got["n_agg"][1] == 0
    if K >= 63:
        assert 0 < got["keep"][0].sum() < K - 2, "the filter keeps some rows and drops some"
    free = check_centroids(hip_device, stats, n_towers, f"K={K} unfiltered", apply_filter=False)
    assert free["keep"][0].sum() == K - min(2, K // 4) and free["keep"][2].sum() == K
    if K >= 63:
        assert free["n_agg"][0] < free["keep"][0].sum(), "some rows merge"
    # the ground truth's side with its own row count: Kg rows against K proposals
    for Kg, gt_n in ((K, [K, K, K + 3]), (max(1, K // 2), [1, 0, max(1, K // 2)])):
        gt, gn = sc.table([sc.random_rows(Kg, 30 + K, extent), sc.random_rows(Kg, 31 + K, extent),
                           sc.random_rows(Kg + 3, 32 + K, extent)], Kg, n_towers=gt_n)
        for cents in (got, free):
            m, want = check_match(hip_device, cents["agg"], cents["n_agg"], cents["status"], gt, gn, f"K={K} Kg={Kg}",
                                  hit_dist=1.0)
            assert m["totals"][1] == 1 or Kg != K      # tile 2 is skipped (both sides overflow at Kg == K)
    # B = 1 with a single row
    one, n1 = sc.table([sc.random_rows(1, 5)], K)
    g1 = check_centroids(hip_device, one, n1, f"K={K} one row", apply_filter=False)
    assert g1["n_agg"].tolist() == [1]


# --------------------------------------------------------------------------- filter edges
def _axes(height_axis, h, p0, p1):
    """a (height, planar 0, planar 1) triple in grid-axis order"""
    out = [0, 0, 0]
    plane = sc.plane_of(height_axis)
    out[height_axis], out[plane[0]], out[plane[1]] = h, p0, p1
    return out


@pytest.mark.parametrize("height_axis", (0, 1, 2))
def test_filter_edges(hip_device, height_axis):
    ax = lambda h, p0, p1: _axes(height_axis, h, p0, p1)   # noqa: E731

    def tower(height, spread0, spread1, c=(1, 1)):
        # integer sums: every quantity of the filter is exact
        return sc.at(ax(7, *c), 1, lo=ax(0, 0, 0), hi=ax(height, spread0, spread1))
    rows = [tower(14, 9, 2),            # height exactly tower_height: kept whatever its spread
            tower(13, 9, 2),            # one below, too wide: dropped
            tower(3, 5, 2),             # spread exactly the threshold: kept
            tower(3, 6, 2),             # one above: dropped
            tower(3, 2, 6),             # (the larger of the two planar extents counts)
            tower(14, 1, 1, c=(3, 4))]  # planar distance^2 exactly rim_sq = 25: kept
    stats, n_towers = sc.table([rows], 8)
    kw = dict(height_axis=height_axis, center=[0.0, 0.0, 0.0], threshold=5.0, tower_height=14.0, radius=15.0)
    got = check_centroids(hip_device, stats, n_towers, "edges", **kw)
    assert got["keep"][0].tolist() == [1, 0, 1, 0, 0, 1, 0, 0]
    # the centroid one ulp outward along the second planar axis: 9 + (4 + ulp)^2 > 25
    s = ax(1.0, 1.0, ULP1)
    moved = check_centroids(hip_device, stats, n_towers, "one ulp outward", voxel_size=s, **kw)
    assert moved["keep"][0].tolist() == [1, 0, 1, 0, 0, 0, 0, 0]
    assert moved["planar"][0, 5, 1] == np.nextafter(4.0, 5.0)
    # radius - 2 * threshold negative: its square is still positive, the rim test still passes inside it
    neg = check_centroids(hip_device, stats, n_towers, "negative rim", **dict(kw, radius=5.0))
    assert (5.0 - 5.0 * 2) ** 2 == 25.0 and neg["keep"][0].tolist() == [1, 0, 1, 0, 0, 1, 0, 0]
    tight = check_centroids(hip_device, stats, n_towers, "rim inside", **dict(kw, radius=14.0))
    assert tight["keep"][0].tolist() == [1, 0, 1, 0, 0, 0, 0, 0]


# --------------------------------------------------------------------------- aggregation
def test_aggregation(hip_device):
    rng = np.random.default_rng(7)
    forty = []
    for _ in range(40):      # mutually within 1.5: every row sums all forty, in id order
        n = int(rng.integers(1, 13))
        forty.append(sc.row(n, [0, int(rng.integers(5 * n, 5 * n + n // 2 + 1)), int(rng.integers(5 * n, 5 * n + n // 2 + 1))]))
    forty.append(sc.row(10, [0, 65, 52]))     # (6.5, 5.2): within 1.5 of some of them only
    tiles = [
        [sc.at((0, 0, 0)), sc.at((0, 0, 1.5), 2), sc.at((0, 0, 3))],                       # the chain A-B-C
        [sc.at((0, 2, 2)), sc.at((5, 2, 2), 2)],                                           # identical planar centroids
        [sc.row(3, [0, 1, 2]), sc.row(7, [0, 3, 5]), sc.row(11, [0, 4, 9]), sc.row(7, [0, 12, 3]), sc.row(11, [0, 30, 13])],
        forty,
        [sc.at((0, 5, 1)), sc.at((0, 5, 9)), sc.at((0, 5, 5)), sc.at((0, 2, 7))],          # equal in column 0: the sort
    ]
    stats, n_towers = sc.table(tiles, 64)
    got = check_centroids(hip_device, stats, n_towers, "aggregation", apply_filter=False)
    assert got["n_agg"][0] == 3 and got["agg"][0, :3].tolist() == [[0.0, 0.75], [0.0, 1.5], [0.0, 2.25]]
    assert got["n_agg"][1] == 1 and got["agg"][1, 0].tolist() == [2.0, 2.0]
    assert got["n_agg"][2] == 3, "denominators 3, 7, 11: means over different members stay distinct rows"
    assert 2 <= got["n_agg"][3] <= 4
    assert got["agg"][4, :4].tolist() == [[2.0, 7.0], [5.0, 1.0], [5.0, 5.0], [5.0, 9.0]] and got["n_agg"][4] == 4
    # exactly min_euc apart: one row; the same pair one ulp further apart: two
    pair, n2 = sc.table([[sc.at((0, 0, 0)), sc.at((0, 0, 1))]], 2)
    exact = check_centroids(hip_device, pair, n2, "exactly min_euc", apply_filter=False, min_euc=1.0)
    assert exact["n_agg"].tolist() == [1] and exact["agg"][0, 0].tolist() == [0.0, 0.5]
    apart = check_centroids(hip_device, pair, n2, "one ulp beyond min_euc", apply_filter=False, min_euc=1.0,
                            voxel_size=(1.0, 1.0, ULP1))
    assert apart["n_agg"].tolist() == [2] and apart["agg"][0].tolist() == [[0.0, 0.0], [0.0, ULP1]]


# --------------------------------------------------------------------------- match
def test_match_edges(hip_device):
    nan = math.nan
    agg = np.array([[[0.0, 0.0], [0.0, 2.0], [nan, nan]],      # two proposals equidistant from the gt row: the lower index
                    [[nan, nan]] * 3,                          # no proposals
                    [[1.0, 1.0], [nan, nan], [nan, nan]]])     # no ground-truth rows
    n_agg = np.array([2, 0, 1], dtype=np.int32)
    gt, gn = sc.table([[sc.at((0, 0, 1))], [sc.at((0, 4, 4)), sc.at((3, 1, 2))], []], 4)
    got, _ = check_match(hip_device, agg, n_agg, np.zeros(3, np.int32), gt, gn, "edges", hit_dist=3.5)
    assert got["match"][0, 0] == 0 and got["dist"][0, 0] == 1.0
    assert got["match"][1].tolist() == [-1, -1, -1, -1] and got["dist"][1, :2].tolist() == [0.0, 0.0]
    assert np.isnan(got["dist"][1, 2:]).all() and np.isnan(got["dist"][2]).all() and (got["match"][2] == -1).all()
    assert dict(zip(sc.TOTAL_NAMES, got["totals"].tolist())) == dict(
        tiles=3, tiles_skipped=0, gt_towers=3, proposals=3, hits=1, misses=2, false_proposals=2, reserved=0)
    # without totals the outputs are the same
    plain = run_match(hip_device, agg, n_agg, np.zeros(3, np.int32), gt, gn, hit_dist=3.5)
    assert all(sc.same_bits(plain[k], got[k]) for k in ("match", "dist", "gt_planar"))


def test_distances_are_numpys_roots(hip_device):
    # 4 x 1024 ground-truth rows with fractional centroids against 8 fractional proposals each: the correctly rounded root
    rng = np.random.default_rng(11)
    agg = np.sort(rng.random((4, 8, 2)) * 64.0, axis=1)
    n_agg = np.full(4, 8, dtype=np.int32)
    gt, gn = sc.table([sc.random_rows(1024, 40 + b, 64) for b in range(4)], 1024)
    got, want = check_match(hip_device, agg, n_agg, np.zeros(4, np.int32), gt, gn, "4096 pairs", hit_dist=8.0)
    assert got["totals"][2] == 4096 and 0 < got["totals"][4] < 4096
    m = got["match"].astype(np.int64)
    d = got["gt_planar"] - np.take_along_axis(agg, m[..., None].repeat(2, axis=2), axis=1)
    assert sc.same_bits(got["dist"], np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]))
    assert len(np.unique(got["dist"])) > 4000 and (got["dist"] != np.round(got["dist"])).all()


# --------------------------------------------------------------------------- totals
def test_totals_accumulate_and_dist_total_is_deterministic(hip_device):
    calls = []
    for seed in (1, 2, 3):
        stats, n_towers = sc.table([sc.random_rows(40, seed), sc.random_rows(20, 50 + seed), sc.random_rows(67, 60 + seed),
                                    sc.random_rows(30, 70 + seed)], 64, n_towers=[40, 20, 67, 30])   # tile 2: rows missing
        gt, gn = sc.table([sc.random_rows(25, 80 + seed, 12), sc.random_rows(9, 90 + seed, 12), sc.random_rows(5, seed, 12),
                           sc.random_rows(35, 95 + seed, 12)], 32, n_towers=[25, 9, 5, 35])          # tile 3: gt rows missing
        cents = run_centroids(hip_device, stats, n_towers, apply_filter=False)
        assert cents["status"].tolist() == [0, 0, 1, 0]
        calls.append((cents["agg"], cents["n_agg"], cents["status"], gt, gn))
    # a proposal that is nearest to a ground-truth row but beyond hit_dist: a miss and a false proposal
    agg = np.array([[[1.0, 1.0], [10.0, 10.0]]])
    gt, gn = sc.table([[sc.at((0, 1, 1)), sc.at((0, 10, 14))]], 2)
    calls.append((agg, np.array([2], np.int32), np.zeros(1, np.int32), gt, gn))
    want_totals = np.zeros(sc.NTOTAL, dtype=np.int64)
    hit_dists = []
    for c in calls:
        w = sc.match_oracle(*c, hit_dist=3.0)
        want_totals += w["totals"]
        hit_dists += w["hit_dists"]
    last = sc.match_oracle(*calls[-1], hit_dist=3.0)["totals"]
    assert last[4] == 1 and last[5] == 1 and last[6] == 1
    runs = []
    for _ in range(2):
        totals = torch.zeros(sc.NTOTAL, dtype=torch.int64, device=hip_device)
        dist_total = torch.zeros(1, dtype=torch.float64, device=hip_device)
        for c in calls:
            run_match(hip_device, *c, hit_dist=3.0, totals=totals, dist_total=dist_total)
        runs.append((totals.cpu().numpy(), dist_total.cpu().numpy()))
    assert np.array_equal(runs[0][0], want_totals) and np.array_equal(runs[1][0], want_totals)
    assert want_totals[1] == 6 and want_totals[0] == 7 and want_totals[4] > 10 and want_totals[7] == 0
    assert want_totals[5] == want_totals[2] - want_totals[4]
    assert sc.same_bits(runs[0][1], runs[1][1]), "dist_total is deterministic"
    ref, bound = sc.dist_total_bound(hit_dists)
    assert ref > 0 and abs(float(runs[0][1][0]) - ref) <= bound


# --------------------------------------------------------------------------- anisotropic voxel size
def test_anisotropic_voxel_size(hip_device):
    s = (1.3, 0.5, 0.75)
    stats, n_towers = sc.table([sc.random_rows(50, 3), sc.random_rows(33, 4)], 64)
    kw = dict(height_axis=1, voxel_size=s, center=[9.0, 3.5, 5.0], threshold=3.0, tower_height=5.0, radius=14.0)
    got = check_centroids(hip_device, stats, n_towers, "anisotropic", **kw)
    assert 0 < got["keep"].sum() < 83
    gt, gn = sc.table([sc.random_rows(20, 5), sc.random_rows(64, 6)], 64)
    m, _ = check_match(hip_device, got["agg"], got["n_agg"], got["status"], gt, gn, "anisotropic", height_axis=1,
                       voxel_size=s, hit_dist=1.0)
    assert 0 < m["totals"][4] < m["totals"][2]


# --------------------------------------------------------------------------- the Python layer
def _metric(**kw):
    args = dict(tau=0.65, eps=1.5, min_points=6, hit_dist=2.0, threshold=2.0, tower_height=3.0, radius=50.0, max_towers=64)
    args.update(kw)
    return sna.TowerDetectionMetrics(**args)


def _oracle_update(pred, gt, metric):
    """the oracle chain on two bool batches, with the metric's settings"""
    _, pn, ps = tc.dbscan_batch(pred, metric.eps, metric.min_points, metric.voxel_size, metric.max_towers)
    _, gn, gs = tc.dbscan_batch(gt, metric.eps, metric.min_points, metric.voxel_size, metric.max_towers)
    s = sc.size_of(metric.voxel_size)
    center = (np.array(pred.shape[1:], dtype=np.float64) - 1.0) / 2.0 * s if metric.center is None else metric.center
    c = sc.centroids_oracle(ps, pn, metric.height_axis, metric.voxel_size, center, metric.apply_filter, metric.threshold,
                            metric.tower_height, metric.radius, metric.min_euc)
    m = sc.match_oracle(c["agg"], c["n_agg"], c["status"], gs, gn, metric.height_axis, metric.voxel_size, metric.hit_dist)
    return c, m


def test_capture_and_replay_on_refilled_buffers(hip_device):
    shape = (16, 16, 70)
    contents = []
    for seeds in ((1, 2), (3, 4)):
        p = np.stack([tc.small_grid(shape, s) for s in seeds])
        g = np.stack([tc.small_grid(shape, s + 10) for s in seeds])
        contents.append((p, g))
    contents[1][0][1] = False
    order = (0, 1, 0)
    eager = _metric().to(hip_device)
    for i in order:
        p, g = contents[i]
        eager.update(torch.from_numpy(p.astype(np.float32)).to(hip_device), torch.from_numpy(g).to(hip_device))
    torch.cuda.synchronize()
    want_totals = np.zeros(sc.NTOTAL, dtype=np.int64)
    hit_dists = []
    for i in order:
        _, m = _oracle_update(*contents[i], eager)
        want_totals += m["totals"]
        hit_dists += m["hit_dists"]
    assert np.array_equal(eager.totals.cpu().numpy(), want_totals)
    assert want_totals[0] == 6 and want_totals[4] > 50 and want_totals[5] > 50 and want_totals[6] > 50
    ref, bound = sc.dist_total_bound(hit_dists)
    assert abs(float(eager.dist_total.item()) - ref) <= bound

    replayed = _metric().to(hip_device)
    buf_p = torch.from_numpy(contents[0][0].astype(np.float32)).to(hip_device)
    buf_g = torch.from_numpy(contents[0][1]).to(hip_device)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        replayed.update(buf_p, buf_g)
    assert replayed.totals.sum().item() == 0, "capturing runs nothing"
    for i in order:
        buf_p.copy_(torch.from_numpy(contents[i][0].astype(np.float32)))
        buf_g.copy_(torch.from_numpy(contents[i][1]))
        graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(replayed.totals, eager.totals)
    assert sc.same_bits(replayed.dist_total.cpu().numpy(), eager.dist_total.cpu().numpy())
    v = replayed.compute()
    assert v["hits"] == want_totals[4] and v["recall"] == want_totals[4] / want_totals[2]
    assert v["mean_error"] == float(eager.dist_total.item()) / want_totals[4]
    replayed.reset()
    assert replayed.totals.sum().item() == 0 and replayed.dist_total.item() == 0.0


def test_end_to_end_on_the_golden_tile(hip_device, golden_dir):
    a = np.load(os.path.join(golden_dir, "ts40k_sample575_full.npz"))["tile"]
    batch = sna.PointBatch.from_tiles([a[:, :3]], [a[:, 3]], device=hip_device)
    grids = sna.voxelize_batch(batch, (64, 64, 64), [15.0], want_occ=True, want_gt_occ=True, occ_dtype=torch.bool)
    gt = grids.gt_occ[:, 0].cpu().numpy() != 0
    # the prediction: the tile OR-ed with itself shifted by one along axis 1, plus a block
    pred = gt.copy()
    pred[:, :, 1:, :] |= gt[:, :, :-1, :]
    pred[:, 40:60, 5:9, 50:54] = True
    _, gn, gs = tc.dbscan_batch(gt, 3.5, 18)
    _, pn, ps = tc.dbscan_batch(pred, 3.5, 18)
    assert gn.tolist() == [1] and pn.tolist() == [2]
    pred_dev = torch.from_numpy(pred.astype(np.float32) * 0.9).to(hip_device)      # a probability grid, tau 0.65
    gt_dev = torch.from_numpy(gt).to(hip_device)
    center = (np.array(gt.shape[1:], dtype=np.float64) - 1.0) / 2.0

    # get_tower_proposals: K8, the filter with threshold = min_dist / 2 in index units, the aggregation
    got = sna.get_tower_proposals(pred_dev, 0.65)
    want = sc.centroids_oracle(ps, pn, 0, None, center, True, 3.5 / 2)
    for name in ("keep", "planar", "agg", "n_agg", "status"):
        assert sc.same_bits(getattr(got, name).cpu().numpy(), want[name]), name
    assert sc.same_bits(got.rows(0), want["agg"][0, :want["n_agg"][0]])

    # compute_euc_dists: no filter
    m = sna.compute_euc_dists(pred_dev, gt_dev, 0.65)
    free = sc.centroids_oracle(ps, pn, 0, None, None, False)
    wm = sc.match_oracle(free["agg"], free["n_agg"], free["status"], gs, gn)
    assert sc.same_bits(m.centroids.agg.cpu().numpy(), free["agg"]) and free["n_agg"].tolist() == [2]
    assert sc.same_bits(m.match.cpu().numpy(), wm["match"]) and sc.same_bits(m.dist.cpu().numpy(), wm["dist"])
    assert sc.same_bits(m.gt_planar.cpu().numpy(), wm["gt_planar"])
    samples = m.sample_distances(0)
    assert len(samples) == 1 and samples[0][2] == wm["dist"][0, 0] and 0.0 < samples[0][2] < 1.0
    assert np.array_equal(samples[0][0], wm["gt_planar"][0, 0]) and np.array_equal(samples[0][1], free["agg"][0, wm["match"][0, 0]])

    # the metric with the reference's thresholds, in index units: whatever the oracle says
    metric = sna.TowerDetectionMetrics(tau=0.65, hit_dist=3.5).to(hip_device)
    metric.update(pred_dev, gt_dev)
    c, wm = _oracle_update(pred, gt, metric)
    assert sc.same_bits(c["agg"], want["agg"])
    assert np.array_equal(metric.totals.cpu().numpy(), wm["totals"])
    ref, bound = sc.dist_total_bound(wm["hit_dists"])
    assert abs(float(metric.dist_total.item()) - ref) <= bound
    v = metric.compute()
    assert v == sna.tower_detection_values(wm["totals"], float(metric.dist_total.item()))
    assert v["tiles"] == 1 and v["gt_towers"] == 1
