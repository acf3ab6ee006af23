"""Nearest neighbours (K21) on the device against the brute-force oracle of knn_cases.py: d2, found, index and mean_dist
bit for bit; the tile statistics within the bound of any summation order; outlier removal, the k-distance curve,
avg_dist_points and a captured call."""
import math
import os

import numpy as np
import pytest
import torch

import scene_net_amd as sna
from scene_net_amd import _hip

import knn_cases as kc

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _batch(tiles):
    """a PointBatch of numpy tiles, empty ones allowed (PointBatch.from_tiles refuses those)"""
    sizes = tuple(len(t) for t in tiles)
    pts = torch.from_numpy(np.ascontiguousarray(np.concatenate([np.asarray(t).reshape(-1, 3) for t in tiles]))).to(_dev())
    offsets = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int64, device=_dev())
    return sna.PointBatch(pts, None, offsets, sizes)


def _host(nb):
    f = lambda t: None if t is None else t.cpu().numpy()   # noqa: E731
    return f(nb.d2), f(nb.found), f(nb.mean_dist), f(nb.index)


def _same(got, want, what=""):
    """bit for bit: d2, found, mean_dist (NaN where the oracle has NaN), index -- whichever the call returned"""
    d2, found, mean, index = got
    assert np.array_equal(d2, want[0]), f"d2 {what}"
    assert np.array_equal(found, want[1]), f"found {what}"
    if mean is not None:
        assert mean.tobytes() == want[2].tobytes() or np.array_equal(mean, want[2], equal_nan=True), f"mean_dist {what}"
        assert np.array_equal(np.isnan(mean), np.isnan(want[2]))
    if index is not None:
        assert np.array_equal(index, want[3]), f"index {what}"


def _run(P, radius, k, **kw):
    return _host(sna.knn_distances(torch.from_numpy(P).to(_dev()), k, radius, **kw))


# ---- blobs: full, partial and empty lists, every k on and between the instantiations -----------------------------------
@pytest.mark.parametrize("k", kc.KS)
@pytest.mark.parametrize("which", range(4))
def test_blobs(which, k):
    P, r = kc.blobs_case(which)[0], kc.BLOB_RADIUS[which]
    want = kc.oracle_of_blobs(which, k)
    _same(_run(P, r, k, want_index=True, want_mean=True), want, "with index and mean")
    got = _run(P, r, k, want_index=False, want_mean=False)
    assert got[2] is None and got[3] is None
    _same(got, want, "without index and mean")


# ---- ties -------------------------------------------------------------------------------------------------------------
def test_ties_break_by_row_index_whatever_the_row_order():
    P = kc.rim_case(0)[0]
    want = kc.knn_oracle(P, 5.0, 16)
    assert ((np.diff(want[0], axis=1) == 0) & np.isfinite(want[0][:, 1:])).sum() > 1000
    _same(_run(P, 5.0, 16, want_index=True), want)
    perm = np.random.default_rng(2).permutation(len(P))
    Pp = np.ascontiguousarray(P[perm])                                # row i of this run is row perm[i] of the first
    d2, found, mean, index = _run(Pp, 5.0, 16, want_index=True)
    _same((d2, found, mean, index), kc.knn_oracle(Pp, 5.0, 16), "permuted: ties by THIS run's row index")
    assert np.array_equal(d2, want[0][perm]) and np.array_equal(found, want[1][perm]), "the distances do not move"
    # at a radius whose whole neighbourhood fits the list, the neighbours are the same points: indices map through perm
    small, small_p = kc.knn_oracle(P, 1.5, 16), _run(Pp, 1.5, 16, want_index=True)
    fits = small_p[1] <= 16
    assert fits.sum() > 300 and (small_p[1] >= 4).sum() > 100
    mapped = np.where(small_p[3] >= 0, perm[small_p[3]], -1)
    assert np.array_equal(np.sort(mapped[fits], axis=1), np.sort(small[3][perm][fits], axis=1))


# ---- cell seams -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_cells,mult", [(1 << 18, 1), (63999, 2)])
def test_pairs_one_radius_apart_across_a_seam(max_cells, mult):
    dims, side = _hip.dbscan_cell_grid(kc.SEAM_BOUNDS, kc.SEAM_EPS, max_cells)
    assert side == mult * kc.SEAM_EPS * (1.0 + 2.0 ** -20) and dims == ((40, 40, 40) if mult == 1 else (20, 20, 20))
    P = kc.seam_case(side)[0]
    lo = torch.from_numpy(kc.SEAM_LO.copy()).to(_dev()).reshape(1, 3)
    for k in (1, 4):
        want = kc.knn_oracle(P, kc.SEAM_EPS, k)
        assert (want[0] == kc.SEAM_EPS ** 2).sum() >= 27
        _same(_run(P, kc.SEAM_EPS, k, want_index=True, lo=lo, extent=(80.0, 80.0, 80.0), max_cells=max_cells), want)


# ---- contraction ------------------------------------------------------------------------------------------------------
def test_the_distance_is_not_contracted():
    P, eps, _, pairs, verdict = kc.contraction_case()
    want = kc.knn_oracle(P, eps, 1)
    assert np.array_equal(want[1][0::2], verdict.astype(np.int32)), "a pair is a neighbour pair iff the plain sum says so"
    _same(_run(P, eps, 1, want_index=True), want)


# ---- any bounds -------------------------------------------------------------------------------------------------------
def test_any_lo_and_any_dims_give_the_same_bits():
    P, r, k = kc.blobs_case(1)[0], kc.BLOB_RADIUS[1], 5
    want = kc.oracle_of_blobs(1, k)
    lo, hi = P.min(axis=0), P.max(axis=0)
    ext = hi - lo
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(_dev()).reshape(1, 3)   # noqa: E731
    ways = {"lo far above: all clamped into the first corner": dict(lo=t(hi + 1e6), extent=tuple(ext)),
            "lo far below: all clamped into the last corner": dict(lo=t(lo - 1e6), extent=tuple(ext)),
            "one cell": dict(lo=t(lo), extent=(0.0, 0.0, 0.0)),
            "a grid ten times the cloud": dict(lo=t(lo - 4.5 * ext), extent=tuple(10.0 * ext))}
    for name, kw in ways.items():
        _same(_run(P, r, k, want_index=True, **kw), want, name)


# ---- tiles ------------------------------------------------------------------------------------------------------------
def test_tiles_never_see_each_other():
    P, r, k = kc.blobs_case(3, 700)[0], 1.6, 4
    one = np.array([[1.0, 2.0, 3.0]]) + kc.ORIGIN
    two = np.array([[1.0, 2.0, 3.0], [1.0, 2.0, 3.0]]) + kc.ORIGIN
    tiles = [P, P, np.zeros((0, 3)), P, one, P, two, P]
    for ez in (False, True):
        want = kc.batch_oracle(tiles, r, k, exclude_zero=ez)
        nb = sna.knn_distances(_batch(tiles), k, r, want_index=True, exclude_zero=ez)
        got = _host(nb)
        _same(got, want, f"exclude_zero={ez}")
        single = kc.knn_oracle(P, r, k, exclude_zero=ez)
        for b in (0, 1, 3, 5, 7):                                    # the same cloud at the same coordinates, five times
            a = int(nb.offsets[b])
            rows = slice(a, a + len(P))
            assert np.array_equal(got[0][rows], single[0]) and np.array_equal(got[1][rows], single[1])
            assert np.array_equal(got[3][rows], np.where(single[3] >= 0, single[3] + a, -1)), "nothing leaks"
        i1, i2 = int(nb.offsets[4]), int(nb.offsets[6])
        assert got[1][i1] == 0 and np.isinf(got[0][i1]).all() and (got[3][i1] == -1).all() and np.isnan(got[2][i1])
        if ez:
            assert got[1][i2:i2 + 2].tolist() == [0, 0] and np.isnan(got[2][i2:i2 + 2]).all()
        else:
            assert got[1][i2:i2 + 2].tolist() == [1, 1] and got[0][i2:i2 + 2, 0].tolist() == [0.0, 0.0]
            assert got[3][i2:i2 + 2, 0].tolist() == [i2 + 1, i2] and got[2][i2:i2 + 2].tolist() == [0.0, 0.0]
        st = nb.stats.cpu().numpy()
        assert st[2].tolist()[:4] == [0.0, 0.0, 0.0, 0.0] and st[2][4] == -np.inf, "the empty tile"
        assert st[4][0] == 0.0 and np.array_equal(st[0], st[1]) and np.array_equal(st[0], st[7])


# ---- chunk edges ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("delta", ["c-1", "c", "c+1", "2c+1"])
def test_chunk_edges(delta):
    c = _hip.knn_chunk_points()
    m = {"c-1": c - 1, "c": c, "c+1": c + 1, "2c+1": 2 * c + 1}[delta]
    P = kc.small_cloud(m, 11 + m)
    want = kc.knn_oracle(P, 1.5, 8)
    assert (want[1] >= 8).any() and (want[1] < 8).any()
    nb = sna.knn_distances(torch.from_numpy(P).to(_dev()), 8, 1.5, want_index=True)
    _same(_host(nb), want)
    _check_stats(nb.stats.cpu().numpy()[0], want[1], want[2], 8)


# ---- non-finite coordinates ---------------------------------------------------------------------------------------------
def test_non_finite_rows_have_no_neighbours_and_are_nobodys():
    P, _, _, odd = kc.nonfinite_case()
    k, r = 4, 1.2
    d2, found, mean, index = _run(P, r, k, want_index=True)
    _same((d2, found, mean, index), kc.knn_oracle(P, r, k), "the oracle takes the comparison literally too")
    assert (found[odd] == 0).all() and np.isinf(d2[odd]).all() and (index[odd] == -1).all() and np.isnan(mean[odd]).all()
    assert not np.isin(index, odd).any(), "in nobody's list"
    fine = np.setdiff1d(np.arange(len(P)), odd)
    sub = kc.knn_oracle(P[fine], r, k)
    assert np.array_equal(d2[fine], sub[0]) and np.array_equal(found[fine], sub[1])
    assert np.array_equal(index[fine], np.where(sub[3] >= 0, fine[sub[3]], -1)), "the finite subset mapped back"
    assert (found[fine] > 0).sum() > 100


# ---- tile statistics ----------------------------------------------------------------------------------------------------
def _check_stats(st, found, mean, k):
    n_valid, n_full, s, sq, mx = kc.tile_stats_oracle(found, mean, k)
    v = mean[found >= 1]
    print(f"stats: n_valid {st[0]} n_full {st[1]} sum {st[2]!r} (fsum {s!r}) sum_sq {st[3]!r} (fsum {sq!r}) max {st[4]!r}")
    assert st[0] == n_valid and st[1] == n_full and st[4] == mx, "counts and max are exact"
    n = max(len(v), 1)
    assert abs(st[2] - s) <= n * 2.0 ** -53 * math.fsum(np.abs(v).tolist())
    assert abs(st[3] - sq) <= n * 2.0 ** -53 * math.fsum((v * v).tolist())


def test_tile_statistics_fixed_order():
    tiles = [kc.blobs_case(2)[0], kc.small_cloud(300, 5), kc.blobs_case(0)[0]]
    k, r = 8, 2.5
    want = [kc.knn_oracle(P, r, k) for P in tiles]
    batch = _batch(tiles)
    a, b = sna.knn_distances(batch, k, r), sna.knn_distances(batch, k, r)
    st = a.stats.cpu().numpy()
    assert st.tobytes() == b.stats.cpu().numpy().tobytes(), "two runs give equal bits"
    for t in range(3):
        _check_stats(st[t], want[t][1], want[t][2], k)
    mean, std, n_valid, n_full = sna.point_spacing(batch, k, r)
    for t in range(3):
        mu, sd = kc.spacing_oracle(want[t][1], want[t][2], k)
        assert abs(float(mean[t]) - mu) <= 1e-12 * mu and abs(float(std[t]) - sd) <= 1e-9 * sd
        assert int(n_valid[t]) == (want[t][1] >= 1).sum() and int(n_full[t]) == (want[t][1] >= k).sum()
    lone = sna.point_spacing(torch.from_numpy(kc.small_cloud(1, 3)).to(_dev()), 1, 1.0)
    assert math.isnan(float(lone[0][0])) and math.isnan(float(lone[1][0])) and int(lone[2][0]) == 0


# ---- outlier removal ----------------------------------------------------------------------------------------------------
def _statistical_keep(found, mean, k, ratio):
    mu, sd = kc.spacing_oracle(found, mean, k)
    thr = mu + ratio * sd
    near = np.abs(mean[found >= 1] - thr) <= 1e-9 * thr
    assert not near.any(), "no row of this set sits on the threshold: the sum's order cannot decide a row"
    with np.errstate(invalid="ignore"):
        return mean <= thr


def test_remove_outliers_both_rules():
    Q = kc.noisy_blobs()
    labels = np.arange(len(Q), dtype=np.float64)
    tiles = [Q, kc.blobs_case(1)[0]]
    k, r, ratio, mn = 8, 2.5, 1.0, 4
    want = [kc.knn_oracle(P, r, k) for P in tiles]
    keep_stat = [_statistical_keep(w[1], w[2], k, ratio) for w in want]
    keep_rad = [w[1] >= mn for w in want]
    assert 0.3 < keep_stat[0].mean() < 0.98 and 0.3 < keep_rad[0].mean() < 0.98
    # one tile with labels
    x, lab = torch.from_numpy(Q).to(_dev()), torch.from_numpy(labels).to(_dev())
    for keep, kw in ((keep_stat[0], dict(k=k, std_ratio=ratio)), (keep_rad[0], dict(min_neighbours=mn))):
        out = sna.remove_outliers(x, radius=r, labels=lab, **kw)
        src = np.flatnonzero(keep)
        assert np.array_equal(out.src.cpu().numpy(), src) and np.array_equal(out.batch.pts.cpu().numpy(), Q[src])
        assert np.array_equal(out.batch.labels.cpu().numpy(), labels[src]) and out.batch.offsets.tolist() == [0, len(src)]
    # the two-tile batch
    batch = _batch(tiles)
    for keeps, kw in ((keep_stat, dict(k=k, std_ratio=ratio)), (keep_rad, dict(min_neighbours=mn))):
        out = sna.remove_outliers(batch, radius=r, **kw)
        src = np.flatnonzero(np.concatenate(keeps))
        assert np.array_equal(out.src.cpu().numpy(), src)
        assert out.batch.offsets.tolist() == [0, int(keeps[0].sum()), int(keeps[0].sum() + keeps[1].sum())]


def test_remove_outliers_captured_with_a_capacity():
    tiles = [kc.noisy_blobs(), kc.blobs_case(1)[0]]
    other = [kc.noisy_blobs(seed=43), kc.blobs_case(1)[0][::-1].copy()]
    r, mn = 2.5, 4
    batch = _batch(tiles)
    total = int(batch.pts.shape[0])
    lo_np = np.stack([np.minimum(t.min(axis=0), o.min(axis=0)) for t, o in zip(tiles, other)])
    hi_np = np.stack([np.maximum(t.max(axis=0), o.max(axis=0)) for t, o in zip(tiles, other)])
    lo, extent = torch.from_numpy(lo_np).to(_dev()), tuple(float(v) for v in (hi_np - lo_np).max(axis=0))
    call = lambda: sna.remove_outliers(batch, radius=r, min_neighbours=mn, capacity=total, lo=lo, extent=extent)  # noqa: E731
    call()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = call()
    for pair in (tiles, other):
        batch.pts.copy_(torch.from_numpy(np.concatenate(pair)).to(_dev()))
        graph.replay()
        torch.cuda.synchronize()
        keep = np.concatenate([kc.knn_oracle(P, r, 1)[1] >= mn for P in pair])
        n = int(out.batch.offsets[-1])
        assert n == keep.sum() and np.array_equal(out.src[:n].cpu().numpy(), np.flatnonzero(keep))
        assert np.array_equal(out.batch.pts[:n].cpu().numpy(), np.concatenate(pair)[keep])


# ---- the mirrors --------------------------------------------------------------------------------------------------------
def test_avg_dist_points_on_the_golden_clouds(golden_dir):
    g = np.load(os.path.join(golden_dir, "avg_dist_points.npz"))
    for name in (str(n) for n in g["names"]):
        xyz, (acc, nd), want = g[name + "_xyz"], g[name + "_args"], float(g[name + "_value"])
        nd, m = int(nd), round(len(xyz) * acc)
        got = sna.avg_dist_points(torch.from_numpy(xyz).to(_dev()), float(acc), nd)
        print(f"{name}: reference {want!r} device {got!r} rel {abs(got - want) / abs(want):.2e}")
        assert abs(got - want) <= kc.avg_dist_bound(m, nd) * abs(want), name
        assert got == kc.avg_dist_points_host(xyz, acc, nd), "parity with this project's own oracle is exact"
        assert sna.avg_dist_points(xyz, float(acc), nd) == got, "a numpy cloud is copied up"
    with pytest.raises(ValueError, match="16"):
        sna.avg_dist_points(torch.from_numpy(g["plain25_xyz"]).to(_dev()), 1.0, 17)


def test_k_distance_curve():
    P, r, k = kc.blobs_case(2)[0], 2.5, 5
    d2, found, _, _ = kc.oracle_of_blobs(2, k)
    want = np.sort(np.sqrt(d2[found >= k, k - 1]))[::-1]
    got = sna.k_distance_curve(torch.from_numpy(P).to(_dev()), k, r).cpu().numpy()
    assert np.array_equal(got, want) and len(got) > 1000


# ---- capture ------------------------------------------------------------------------------------------------------------
def test_captured_call_follows_the_buffers():
    P, Q = kc.blobs_case(2)[0], kc.blobs_case(3)[0]
    r, k = 2.5, 8
    x = torch.from_numpy(P).to(_dev())
    both = np.concatenate([P, Q])
    lo = torch.from_numpy(both.min(axis=0)).to(_dev()).reshape(1, 3)
    extent = tuple(float(v) for v in both.max(axis=0) - both.min(axis=0))
    batch = sna.PointBatch(x, None, torch.tensor([0, len(P)], dtype=torch.int64, device=_dev()), (len(P),))
    call = lambda: sna.knn_distances(batch, k, r, want_index=True, lo=lo, extent=extent)   # noqa: E731
    call()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        nb = call()
    graph.replay()
    torch.cuda.synchronize()
    _same(_host(nb), kc.oracle_of_blobs(2, k), "the capture's own cloud")
    x.copy_(torch.from_numpy(Q).to(_dev()))
    graph.replay()
    torch.cuda.synchronize()
    want = kc.knn_oracle(Q, r, k)
    _same(_host(nb), want, "a second cloud copied into the same buffers")
    _check_stats(nb.stats.cpu().numpy()[0], want[1], want[2], k)


def test_captured_calls_replayed_back_to_back():
    """several captured calls on ONE workspace -- the whole call and its launch prefixes, as tools/knn_bench.py holds them --
    replayed back to back with no synchronise in between: every replay of the whole call leaves the oracle's bits.  (Each
    replay must zero the populations the one before left behind.)"""
    P, r, k = kc.blobs_case(2)[0], 2.5, 8
    want = kc.oracle_of_blobs(2, k)
    x = torch.from_numpy(P).to(_dev())
    offsets = torch.tensor([0, len(P)], dtype=torch.int64, device=_dev())
    lo = torch.from_numpy(P.min(axis=0)).to(_dev()).reshape(1, 3)
    dims, side = _hip.dbscan_cell_grid([0.0, 0.0, 0.0] + [float(v) for v in P.max(axis=0) - P.min(axis=0)], r, 1 << 12)
    mult = int(round(side / (r * (1.0 + 2.0 ** -20))))
    ws = torch.empty(_hip.knn_ws_bytes(len(P), 1, dims[0] * dims[1] * dims[2]) // 8, dtype=torch.int64, device=_dev())
    d2 = torch.empty((len(P), k), dtype=torch.float64, device=_dev())
    found = torch.empty(len(P), dtype=torch.int32, device=_dev())
    mean = torch.empty(len(P), dtype=torch.float64, device=_dev())
    index = torch.empty((len(P), k), dtype=torch.int64, device=_dev())

    def call(launches=None):
        _hip.knn_points(x, offsets, r, k, lo, dims, mult, ws, d2, found, mean, index, launches=launches)
    graphs = []
    for launches in (None, (1, 1), (1, 2), (1, 3), (4, 4)):
        call()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            call(launches)
        graphs.append(g)
    for _ in range(2):
        for g in graphs[1:]:
            for _ in range(3):
                g.replay()
        found.zero_()
        for _ in range(3):
            graphs[0].replay()
        torch.cuda.synchronize()
        _same((d2.cpu().numpy(), found.cpu().numpy(), mean.cpu().numpy(), index.cpu().numpy()), want)
    with pytest.raises(_hip.HipLibraryError):
        call((0, 2))
