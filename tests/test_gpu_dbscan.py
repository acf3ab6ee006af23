"""Point DBSCAN (K10) on the device against the numpy oracle of dbscan_cases.py, bit for bit: sel, cluster, n_clusters,
stats and n_sel of every case."""
import os

import numpy as np
import pytest
import torch

import scene_net_amd as sna
from scene_net_amd import _hip

import dbscan_cases as dc

pytestmark = pytest.mark.gpu
SENTINEL = -77


def _embed(P, seed, others=700):
    """(scan, labels): P's rows labelled 15 in their order, interleaved with `others` rows of other labels and NaN"""
    rng = np.random.default_rng(seed)
    n = len(P) + others
    at = np.sort(rng.choice(n, len(P), replace=False))
    scan = dc.ORIGIN + rng.random((n, 3)) * 50.0
    labels = rng.choice(np.array([2.0, 16.0, np.nan]), n)
    scan[at], labels[at] = P, dc.TOWER
    return scan, labels


def _check(out, P, eps, mp, labels=None, keep=None, oracle=None, max_clusters=64):
    """every output of cluster_points (exact path) against the oracle over the selected points"""
    sel_ref = dc.isin_positions(labels, keep)
    Q = P if sel_ref is None else P[sel_ref]
    cluster, K, stats, core = oracle if oracle is not None else dc.dbscan_oracle(Q, eps, mp)
    assert int(out.n_sel) == len(Q) and int(out.status) == 0
    if sel_ref is None:
        assert out.sel is None
    else:
        assert np.array_equal(out.sel.cpu().numpy(), sel_ref)
    assert np.array_equal(out.cluster.cpu().numpy(), cluster)
    assert int(out.n_clusters) == K
    want = np.zeros((max_clusters, 3), dtype=np.int64)
    rows = min(K, max_clusters)
    want[:rows] = stats[:rows]
    if sel_ref is not None:
        want[:rows, 2] = sel_ref[stats[:rows, 2]]
    assert np.array_equal(out.stats.cpu().numpy(), want)
    return cluster, K, core


def _run(dev, P, eps, mp, labels=None, keep=None, **kw):
    return sna.cluster_points(torch.from_numpy(P).to(dev), eps, mp, labels=None if labels is None else
                              torch.from_numpy(labels).to(dev), keep=keep, **kw)


@pytest.mark.parametrize("which", range(4))
def test_blobs_with_noise(hip_device, which):
    P, eps, mp = dc.blobs_case(which)
    scan, labels = _embed(P, which)
    out = _run(hip_device, scan, eps, mp, labels, [dc.TOWER])
    _check(out, scan, eps, mp, labels, [dc.TOWER], oracle=dc.oracle_of_blobs(which))
    towers = out.towers()
    cluster, K = dc.oracle_of_blobs(which)[:2]
    assert len(towers) == K
    for k in range(K):
        assert np.array_equal(towers[k].cpu().numpy(), P[cluster == k])
        assert np.array_equal(out.src(k).cpu().numpy(), dc.isin_positions(labels, [dc.TOWER])[cluster == k])


@pytest.mark.parametrize("shift", (0, 1, -1))
def test_pairs_on_the_rim(hip_device, shift):
    P, eps, mp = dc.rim_case(shift)
    _check(_run(hip_device, P, eps, mp), P, eps, mp)


def test_contraction(hip_device):
    P, eps, mp, pairs, verdict = dc.contraction_case()
    cluster, K, core = _check(_run(hip_device, P, eps, mp, max_clusters=256), P, eps, mp, max_clusters=256)
    assert K == verdict.sum() and np.array_equal(cluster[::2] >= 0, verdict)


@pytest.mark.parametrize("max_cells,clamped", [(1 << 18, False), (64, False), (27, False), (1 << 18, True)])
def test_cell_seams(hip_device, max_cells, clamped):
    dims, side = _hip.dbscan_cell_grid(dc.SEAM_BOUNDS, dc.SEAM_EPS, max_cells)
    P, eps, mp = dc.seam_case(side)
    bounds = dc.SEAM_BOUNDS + (1000.0 if clamped else 0.0)      # (clamped: the bounds contain none of the points)
    out = _run(hip_device, P, eps, mp, capacity=len(P), bounds=bounds.tolist(), max_cells=max_cells)
    _check(out, P, eps, mp)


@pytest.mark.parametrize("order", ("ascending", "descending", "shuffled"))
def test_chain(hip_device, order):
    P, eps, mp = dc.chain_case(order)
    cluster, K, core = _check(_run(hip_device, P, eps, mp), P, eps, mp)
    assert K == 1 and (~core).sum() == 2


@pytest.mark.parametrize("order", ("AXB", "BXA", "XBA", "XAB"))
def test_shared_border(hip_device, order):
    P, eps, mp, x = dc.shared_border_case(order)
    cluster, K, core = _check(_run(hip_device, P, eps, mp), P, eps, mp)
    assert K == 2 and cluster[x] == 0


def test_min_points_extremes(hip_device):
    P = dc.blobs_case(2)[0][:600].copy()
    P[17, 1] = np.nan
    cluster, K, core = _check(_run(hip_device, P, 1.6, 1, max_clusters=512), P, 1.6, 1, max_clusters=512)
    assert core.sum() == 599 and cluster[17] == -1, "every finite point is core"
    cluster, K, core = _check(_run(hip_device, P, 1.6, 601), P, 1.6, 601)
    assert K == 0 and (cluster == -1).all()


def test_degenerate_inputs(hip_device):
    P = np.tile(dc.ORIGIN + np.array([1.5, 2.5, 3.5]), (400, 1))
    cluster, K, core = _check(_run(hip_device, P, 10.0, 300), P, 10.0, 300)
    assert K == 1 and core.all()
    one = P[:1]
    assert _check(_run(hip_device, one, 2.0, 1), one, 2.0, 1)[1] == 1
    assert _check(_run(hip_device, one, 2.0, 2), one, 2.0, 2)[1] == 0
    # m = 0: nothing is selected
    scan, labels = _embed(P[:5], 3, others=40)
    out = _run(hip_device, scan, 2.0, 3, labels, [99.0])
    assert int(out.n_sel) == 0 and int(out.n_clusters) == 0 and int(out.status) == 0 and out.towers() == []
    assert out.cluster.numel() == 0 and not out.stats.any()
    # ... and the entry itself writes no label
    out = _run(hip_device, scan, 2.0, 3, labels, [99.0], capacity=8, bounds=dc.SEAM_BOUNDS.tolist())
    assert int(out.n_sel) == 0 and int(out.n_clusters) == 0 and int(out.status) == 0 and not out.stats.any()
    d_pts = torch.from_numpy(scan).to(hip_device)
    cl = torch.full((8,), SENTINEL, dtype=torch.int32, device=hip_device)
    nc, st = torch.full((1,), SENTINEL, dtype=torch.int32, device=hip_device), torch.ones(1, dtype=torch.int32, device=hip_device)
    stats = torch.full((4, 3), SENTINEL, dtype=torch.int64, device=hip_device)
    ws = torch.empty(_hip.dbscan_ws_bytes(8, 64) // 8, dtype=torch.int64, device=hip_device)
    _hip.dbscan_points(d_pts, torch.zeros(8, dtype=torch.int64, device=hip_device), out.n_sel, dc.SEAM_BOUNDS.tolist(), 2.0, 3,
                       64, 4, ws, cl, nc, stats, st)
    assert (cl == SENTINEL).all() and int(nc) == 0 and int(st) == 0 and not stats.any()


def test_non_finite_inputs(hip_device):
    P, labels, keep, odd = dc.nonfinite_case()
    out = _run(hip_device, P, 1.2, 5, labels, keep)
    cluster, K, core = _check(out, P, 1.2, 5, labels, keep)
    sel = dc.isin_positions(labels, keep)
    is_odd = np.isin(sel, odd)
    assert is_odd.sum() == 12 and (cluster[is_odd] == -1).all(), "NaN, inf and 1e300 points are noise"
    assert np.array_equal(dc.dbscan_oracle(P[sel][~is_odd], 1.2, 5)[0], cluster[~is_odd]), "the others are unchanged"
    # the box of the selection: finite coordinates only
    d_pts, d_lab = torch.from_numpy(P).to(hip_device), torch.from_numpy(labels).to(hip_device)
    ws = torch.empty(_hip.points_select_ws_bytes(len(P)) // 8, dtype=torch.int64, device=hip_device)
    n_sel, bbox = torch.zeros(1, dtype=torch.int64, device=hip_device), torch.zeros(6, dtype=torch.float64, device=hip_device)
    _hip.points_select(d_pts, d_lab, torch.tensor(keep, dtype=torch.float64, device=hip_device), ws, None, n_sel, bbox)
    assert int(n_sel) == len(sel) and np.array_equal(bbox.cpu().numpy(), dc.finite_bbox(P[sel]))


def _cloud(m, seed):
    return dc.small_cloud(m, seed, spread=(m / 1.4) ** (1.0 / 3.0))


@pytest.mark.parametrize("m", (255, 256, 257, 1023, 1024, 1025))
def test_position_chunk_seams(hip_device, m):
    assert _hip.dbscan_chunk_points() == 256 and _hip.points_select_chunk_points() == 1024
    P = _cloud(m, m)
    cluster, K, core = _check(_run(hip_device, P, 1.0, 4), P, 1.0, 4)
    assert K >= 1 and (cluster < 0).any() and core.any()


@pytest.mark.parametrize("n", (1023, 1024, 1025, 2048, 2049))
def test_scan_chunk_seams(hip_device, n):
    P = _cloud(n, n)
    labels = np.random.default_rng(n).choice(np.array([15.0, 2.0]), n, p=[0.7, 0.3])
    labels[[0, n - 1]] = 15.0
    if n > 1024:
        labels[[1023, 1024]] = 15.0
    _check(_run(hip_device, P, 1.2, 4, labels, [15.0]), P, 1.2, 4, labels, [15.0])


def test_select_prefix_carries_into_the_second_scan_tile(hip_device):
    """The select's prefix kernel is one workgroup of 1024 threads, one chunk of 1024 points each: one chunk more than that
    and a little, so the prefixes of chunk 1024 and n_sel hold a carry."""
    c = _hip.points_select_chunk_points()
    tile = 1024                                      # kScanThreads of cell_grid.h
    n = (tile + 1) * c + 3
    rng = np.random.default_rng(1025)
    P = dc.ORIGIN + rng.random((n, 3)) * 50.0
    P[rng.random(n) < 0.001, 1] = np.nan             # left out of the box
    P[[7, n - 2], 2] = [np.inf, -np.inf]
    labels = rng.choice(np.array([15.0, 2.0, 16.0, np.nan]), n)
    labels[[tile * c - 1, tile * c, n - 1]] = [15.0, 16.0, 15.0]
    keep = [15.0, 16.0]
    want = np.nonzero(np.isin(labels, keep))[0]
    assert (want < tile * c).sum() > 0.4 * tile * c and (want >= tile * c).sum() > 300      # selected on both sides
    d_pts, d_lab = torch.from_numpy(P).to(hip_device), torch.from_numpy(labels).to(hip_device)
    ws = torch.empty(_hip.points_select_ws_bytes(n) // 8, dtype=torch.int64, device=hip_device)
    sel = torch.full((len(want) + 50,), SENTINEL, dtype=torch.int64, device=hip_device)
    n_sel, bbox = torch.zeros(1, dtype=torch.int64, device=hip_device), torch.zeros(6, dtype=torch.float64, device=hip_device)
    _hip.points_select(d_pts, d_lab, torch.tensor(keep, dtype=torch.float64, device=hip_device), ws, sel, n_sel, bbox,
                       capacity=len(want) + 50)
    assert int(n_sel) == len(want)
    assert np.array_equal(sel[:len(want)].cpu().numpy(), want) and (sel[len(want):] == SENTINEL).all()
    Q = P[want]
    finite = np.where(np.isfinite(Q), Q, np.nan)
    assert np.array_equal(bbox.cpu().numpy(), np.concatenate([np.nanmin(finite, axis=0), np.nanmax(finite, axis=0)]))
    assert np.array_equal(bbox.cpu().numpy(), dc.finite_bbox(Q))


def test_capacity_and_max_clusters(hip_device):
    P, eps, mp = dc.blobs_case(1)
    scan, labels = _embed(P, 11)
    sel_ref = dc.isin_positions(labels, [dc.TOWER])
    capacity = 1000
    d_pts, d_lab = torch.from_numpy(scan).to(hip_device), torch.from_numpy(labels).to(hip_device)
    keep = torch.tensor([dc.TOWER], dtype=torch.float64, device=hip_device)
    rows = capacity + 50
    sel = torch.full((rows,), SENTINEL, dtype=torch.int64, device=hip_device)
    cl = torch.full((rows,), SENTINEL, dtype=torch.int32, device=hip_device)
    n_sel, bbox = torch.zeros(1, dtype=torch.int64, device=hip_device), torch.zeros(6, dtype=torch.float64, device=hip_device)
    nc, st = torch.zeros(1, dtype=torch.int32, device=hip_device), torch.zeros(1, dtype=torch.int32, device=hip_device)
    stats = torch.full((64, 3), SENTINEL, dtype=torch.int64, device=hip_device)
    ws = torch.empty(_hip.points_select_ws_bytes(len(scan)) // 8, dtype=torch.int64, device=hip_device)
    _hip.points_select(d_pts, d_lab, keep, ws, sel, n_sel, bbox, capacity=capacity)
    box = dc.finite_bbox(P)
    dims, _ = _hip.dbscan_cell_grid(box, eps, 1 << 18)
    ws = torch.empty(_hip.dbscan_ws_bytes(capacity, int(np.prod(dims))) // 8, dtype=torch.int64, device=hip_device)
    _hip.dbscan_points(d_pts, sel, n_sel, box.tolist(), eps, mp, 1 << 18, 64, ws, cl, nc, stats, st, capacity=capacity)
    assert int(n_sel) == 1900 and int(st) == 1, "n_sel is true, status bit 0 is raised"
    assert np.array_equal(bbox.cpu().numpy(), box)
    assert np.array_equal(sel[:capacity].cpu().numpy(), sel_ref[:capacity]) and (sel[capacity:] == SENTINEL).all()
    cluster, K, want, core = dc.dbscan_oracle(P[:capacity], eps, mp)
    assert np.array_equal(cl[:capacity].cpu().numpy(), cluster) and (cl[capacity:] == SENTINEL).all()
    assert int(nc) == K
    want[:, 2] = sel_ref[want[:, 2]]
    assert np.array_equal(stats[:K].cpu().numpy(), want) and not stats[K:].any()
    with pytest.raises(sna.HipLibraryError, match="capacity"):
        sna.cluster_points(d_pts, eps, mp, labels=d_lab, keep=keep, capacity=capacity, bounds=box.tolist()).towers()
    # max_clusters below K: the labels and n_clusters are whole, the stats stop
    P, eps, mp = dc.blobs_case(3)
    K = dc.oracle_of_blobs(3)[1]
    assert K > 5
    _check(_run(hip_device, P, eps, mp, max_clusters=5), P, eps, mp, oracle=dc.oracle_of_blobs(3), max_clusters=5)


def test_captured_replay(hip_device):
    cases = [_embed(dc.blobs_case(w)[0][:1500], 20 + w) for w in (1, 2)]
    eps, mp = 2.5, 8
    n = len(cases[0][0])
    bounds = [dc.ORIGIN[0] - 100, dc.ORIGIN[1] - 100, dc.ORIGIN[2] - 100, dc.ORIGIN[0] + 200, dc.ORIGIN[1] + 200, dc.ORIGIN[2] + 200]
    d_pts = torch.zeros((n, 3), dtype=torch.float64, device=hip_device)
    d_lab = torch.zeros(n, dtype=torch.float64, device=hip_device)
    keep = torch.tensor([dc.TOWER], dtype=torch.float64, device=hip_device)
    d_pts.copy_(torch.from_numpy(cases[0][0]))
    d_lab.copy_(torch.from_numpy(cases[0][1]))
    sna.cluster_points(d_pts, eps, mp, labels=d_lab, keep=keep, capacity=1600, bounds=bounds)   # (eager first: kernels are loaded)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = sna.cluster_points(d_pts, eps, mp, labels=d_lab, keep=keep, capacity=1600, bounds=bounds)
    for scan, labels in (cases[0], cases[1], cases[0]):
        d_pts.copy_(torch.from_numpy(scan))
        d_lab.copy_(torch.from_numpy(labels))
        graph.replay()
        torch.cuda.synchronize()
        sel_ref = dc.isin_positions(labels, [dc.TOWER])
        cluster, K, stats, core = dc.dbscan_oracle(scan[sel_ref], eps, mp)
        assert K > 1 and int(out.n_sel) == 1500 and int(out.status) == 0 and int(out.n_clusters) == K
        assert np.array_equal(out.sel[:1500].cpu().numpy(), sel_ref)
        assert np.array_equal(out.cluster[:1500].cpu().numpy(), cluster)
        stats[:, 2] = sel_ref[stats[:, 2]]
        assert np.array_equal(out.stats[:K].cpu().numpy(), stats) and not out.stats[K:].any()


# ---- end to end ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden_tile(golden_dir):
    return np.load(os.path.join(golden_dir, "ts40k_sample575_full.npz"))["tile"]


def _same(a, b):
    return a.shape == b.shape and np.array_equal(a.cpu().numpy().view(np.int64), b.cpu().numpy().view(np.int64))


def test_golden_tile_end_to_end(hip_device, golden_tile):
    xyz = torch.from_numpy(np.ascontiguousarray(golden_tile[:, :3])).to(hip_device)
    classes = torch.from_numpy(np.ascontiguousarray(golden_tile[:, 3])).to(hip_device)
    T = dc.golden_towers(golden_tile)
    picked, all_classes = sna.select_object(xyz, classes, [15])
    assert np.array_equal(picked.cpu().numpy(), T) and _same(all_classes, classes)
    for eps, mp, K, cores in ((10, 300, 1, 700), (1.0, 10, 6, 753)):
        cluster, k, stats, core = dc.dbscan_oracle(T, eps, mp)
        assert (k, int(core.sum())) == (K, cores)
        towers = sna.extract_towers(picked, eps, mp)
        assert len(towers) == K
        for j in range(K):
            assert np.array_equal(towers[j].cpu().numpy(), T[cluster == j])
        out = sna.cluster_points(xyz, eps, mp, labels=classes, keep=[15])
        _check(out, golden_tile[:, :3].copy(), eps, mp, golden_tile[:, 3].copy(), [15.0], oracle=(cluster, k, stats, core))
    cluster = dc.dbscan_oracle(T, 10, 300)[0]
    assert (cluster == 0).sum() == 776
    given = [torch.from_numpy(T[cluster == 0]).to(hip_device)]
    got, want = sna.crop_tower_samples(xyz, classes), sna.crop_tower_samples(xyz, classes, given)
    assert len(got) == len(want) == 1 and got[0].shape[0] > 776 and _same(got[0], want[0])
    got = sna.crop_tower_samples(xyz, classes, radius=7.5, obj_class=[15], eps=1.0, min_points=10)
    cluster = dc.dbscan_oracle(T, 1.0, 10)[0]
    want = sna.crop_tower_samples(xyz, classes, [torch.from_numpy(T[cluster == j]).to(hip_device) for j in range(6)], 7.5)
    assert len(got) == len(want) == 6 and all(_same(a, b) for a, b in zip(got, want))
    assert sna.crop_two_towers_samples(xyz, classes) == [], "one tower: no pair"


def test_two_towers_samples_on_three_towers(hip_device):
    rng = np.random.default_rng(41)
    centres = np.array([[20.0, 20.0], [70.0, 25.0], [75.0, 90.0]])
    parts, labels = [], []
    for c in centres:
        parts.append(np.column_stack([c + rng.standard_normal((400, 2)) * 1.2, rng.random(400) * 16.0]))
        labels.append(np.full(400, 15.0))
    parts.append(np.column_stack([rng.random((2600, 2)) * 110.0, rng.random(2600) * 2.0]))
    labels.append(rng.choice(np.array([2.0, 3.0]), 2600))
    order = rng.permutation(3800)
    scan = np.ascontiguousarray((dc.ORIGIN + np.concatenate(parts))[order])
    lab = np.concatenate(labels)[order]
    T = scan[lab == 15.0]
    cluster, K, stats, core = dc.dbscan_oracle(T, 10, 300)
    assert K == 3 and (cluster >= 0).all()
    xyz, classes = torch.from_numpy(scan).to(hip_device), torch.from_numpy(lab).to(hip_device)
    towers = [torch.from_numpy(T[cluster == k]).to(hip_device) for k in range(K)]
    # the reference's composition (pcd_processing.py:775-794) over the oracle's towers
    means = np.array([np.mean(T[cluster == k], axis=0) for k in range(K)])
    want = []
    for i in range(K):
        eucs = np.array([np.linalg.norm(means[i] - means[j]) for j in range(K)])
        idx = int(np.argmin(eucs[eucs > 0]))
        if idx >= i:
            idx += 1
        crop2, crop2_cl = sna.crop_two_towers(xyz, classes, towers[i], towers[idx])
        if len(crop2) == 0:
            continue
        pieces = [torch.cat([crop2, crop2_cl.to(torch.float64)[:, None]], dim=1)]
        for t in (towers[i], towers[idx]):
            p, c = sna.crop_tower_radius(xyz, classes, t)
            pieces.append(torch.cat([p, c.to(torch.float64)[:, None]], dim=1))
        want.append(torch.cat(pieces))
    got = sna.crop_two_towers_samples(xyz, classes)
    assert len(got) == len(want) == 3 and all(_same(a, b) for a, b in zip(got, want))
    assert all(g.shape[0] > 800 for g in got)
