"""Neighbourhood shapes (K22) on the device against the oracle of shape_cases.py: count and moments bit for bit, eig, normal,
axis and feat bit for bit against the numpy restatement of the solver, NaN patterns equal; the Python layer on top."""
import numpy as np
import pytest
import torch

import scene_net_amd as sna
from scene_net_amd import _hip

import shape_cases as sc

pytestmark = pytest.mark.gpu
NAMES = ("count", "moments", "eig", "normal", "axis", "feat")


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def _batch(tiles, pad=0):
    """a PointBatch of numpy tiles, empty ones allowed, with `pad` rows beyond offsets[B] that no tile owns"""
    sizes = tuple(len(t) for t in tiles)
    parts = [np.asarray(t, dtype=np.float64).reshape(-1, 3) for t in tiles] + [np.full((pad, 3), 7.0)]
    offsets = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int64, device=_dev())
    return sna.PointBatch(_up(np.concatenate(parts)), None, offsets, sizes)


def _host(sh):
    return tuple(None if t is None else t.cpu().numpy() for t in (sh.count, sh.moments, sh.eig, sh.normal, sh.axis, sh.feat))


def _bits(a):
    return a.view(np.int64) if a.dtype == np.float64 else a


def _same(got, want, what=""):
    """bit for bit, NaN patterns included, whichever outputs the call returned"""
    for name, g, w in zip(NAMES, got, want):
        if g is None:
            continue
        assert g.shape == w.shape and g.dtype == w.dtype, f"{name} {what}: {g.shape} {g.dtype}"
        bad = np.flatnonzero((_bits(g) != _bits(w)).reshape(len(g), -1).any(axis=1))
        assert bad.size == 0, f"{name} {what}: {bad.size} rows differ, first {bad[0]}: {g[bad[0]]!r} != {w[bad[0]]!r}"


def _run(P, radius, **kw):
    return _host(sna.shape_features(_up(P), radius, **kw))


# ---- blobs at UTM offsets ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", range(4))
def test_blobs(which):
    want = sc.oracle_of_blobs(which)
    assert (want[0] >= 3).sum() > 1000 and (want[0] < 3).sum() > 100
    _same(_run(sc.blobs_case(which)[0], sc.BLOB_RADIUS[which]), want)


# ---- cell seams --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_cells,mult", [(1 << 18, 1), (63999, 2)])
def test_pairs_one_radius_apart_across_a_seam(max_cells, mult):
    import knn_cases as kc
    dims, side = _hip.dbscan_cell_grid(kc.SEAM_BOUNDS, kc.SEAM_EPS, max_cells)
    assert side == mult * kc.SEAM_EPS * (1.0 + 2.0 ** -20) and dims == ((40, 40, 40) if mult == 1 else (20, 20, 20))
    P = sc.seam_case(side)[0]
    want = sc.shape_oracle(P, kc.SEAM_EPS)
    assert (np.abs(want[1][:, :3]) == 65536).any(axis=1).sum() >= 54, "members exactly one radius away: f = 65536"
    assert (want[0] >= 3).sum() >= 27
    _same(_run(P, kc.SEAM_EPS, lo=_up(kc.SEAM_LO).reshape(1, 3), extent=(80.0, 80.0, 80.0), max_cells=max_cells), want)


# ---- the grid and the order of the rows do not show ----------------------------------------------------------------------
def test_any_grid_and_any_row_order_give_the_same_bits():
    P, r = sc.blobs_case(1)[0], sc.BLOB_RADIUS[1]
    want = sc.oracle_of_blobs(1)
    lo = _up(P.min(axis=0)).reshape(1, 3)
    _same(_run(P, r, lo=lo, extent=(0.0, 0.0, 0.0)), want, "dims (1, 1, 1): brute force")
    _same(_run(P, r, lo=_up(P.max(axis=0) + 1e6).reshape(1, 3), extent=tuple(P.max(axis=0) - P.min(axis=0))), want, "all clamped")
    perm = np.random.default_rng(2).permutation(len(P))
    _same(_run(P[perm], r), tuple(w[perm] for w in want), "rows permuted: the outputs permute")


# ---- rounding ----------------------------------------------------------------------------------------------------------
def test_offsets_half_way_round_to_even():
    P, r = sc.tie_case()
    want = sc.shape_oracle(P, r)
    assert want[0][0] == len(P)
    _same(_run(P, r), want)


def test_moments_are_64_bit_wide():
    P, r = sc.rim_ring_case()
    want = sc.shape_oracle(P, r)
    assert want[0][0] == len(P) and want[1][0, 3] > 2 ** 41 and (want[1][:, 3:] > 2 ** 32).any(axis=1).sum() > 2000
    _same(_run(P, r), want)


# ---- degenerate neighbourhoods -------------------------------------------------------------------------------------------
def test_collinear_planar_and_coincident_sets():
    line, plane = sc.line_lattice(), sc.plane_lattice()
    wl, wp = sc.shape_oracle(line, 2.0), sc.shape_oracle(plane, 2.0)     # 65536 / 2: every offset is an integer as it stands
    assert (wl[0] >= 3).all() and np.all(wl[5][:, 0] > 1.0 - 1e-12), "linearity 1 up to the solver's rounding"
    assert (wp[0] >= 3).all() and np.all(wp[5][:, 2] < 1e-12), "no scattering"
    _same(_run(line, 2.0), wl, "collinear")
    _same(_run(plane, 2.0), wp, "planar")
    same = np.repeat(sc.ORIGIN[None, :] + 0.25, 40, axis=0)
    got = _run(same, 1.0)
    _same(got, sc.shape_oracle(same, 1.0), "coincident")
    assert (got[0] == 40).all() and (got[1] == 0).all() and all(np.isnan(g).all() for g in got[2:]), "l2 == 0 gives NaN"


@pytest.mark.parametrize("min_points", [3, 5])
def test_rows_with_few_neighbours(min_points):
    P, r = sc.few_neighbours_case()
    want = sc.shape_oracle(P, r, min_points)
    assert sorted(set(want[0].tolist())) == [1, 2, 3, 4, 5]
    assert np.array_equal(np.isnan(want[2][:, 0]), want[0] < min_points)
    _same(_run(P, r, min_points=min_points), want)


def test_non_finite_rows_have_no_neighbours_and_are_nobodys():
    P, _, _, odd = sc.nonfinite_case()
    want = sc.shape_oracle(P, 1.2)
    got = _run(P, 1.2)
    _same(got, want, "the oracle takes the comparison literally too")
    huge = np.abs(P[odd]).max(axis=1) == 1e300                        # finite: its own neighbour, nobody else's
    assert np.array_equal(got[0][odd], huge.astype(np.int32)) and (got[1][odd] == 0).all() and np.isnan(got[5][odd]).all()
    fine = np.setdiff1d(np.arange(len(P)), odd)
    _same(tuple(g[fine] for g in got), sc.shape_oracle(P[fine], 1.2), "the finite subset alone")


# ---- batches -------------------------------------------------------------------------------------------------------------
def test_tiles_never_see_each_other():
    P, r = sc.blobs_case(3, 700)[0], 1.6
    one = np.array([[1.0, 2.0, 3.0]]) + sc.ORIGIN
    tiles = [P, P, np.zeros((0, 3)), P, one, np.zeros((0, 3))]
    want = sc.batch_oracle(tiles, r, pad=5)
    sh = sna.shape_features(_batch(tiles, pad=5), r)
    got = _host(sh)
    _same(got, want)
    single = sc.shape_oracle(P, r)
    for b in (0, 1, 3):                                              # the same cloud at the same coordinates, three times
        a = int(sh.offsets[b])
        _same(tuple(g[a:a + len(P)] for g in got), single, f"tile {b}: nothing leaks")
    assert (got[0][-5:] == 0).all() and (got[1][-5:] == 0).all() and np.isnan(got[2][-5:]).all(), "rows no tile owns"


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_chunk_edges(delta):
    m = _hip.shape_chunk_points() + delta
    tiles = [sc.small_cloud(m, 11 + m), sc.small_cloud(m, 12 + m)]
    want = sc.batch_oracle(tiles, 1.5)
    assert (want[0] >= 3).sum() > 200
    _same(_host(sna.shape_features(_batch(tiles), 1.5)), want)


# ---- nullable outputs ------------------------------------------------------------------------------------------------------
def test_every_output_left_out_in_turn():
    P, r = sc.blobs_case(2)[0], sc.BLOB_RADIUS[2]
    want = sc.oracle_of_blobs(2)
    all_four = ("eig", "normal", "axis", "feat")
    for out in all_four:
        got = _run(P, r, want=tuple(w for w in all_four if w != out))
        assert got[NAMES.index(out)] is None and sum(g is None for g in got) == 1
        _same(got, want, f"without {out}")
    got = _run(P, r, want=(), want_moments=False)
    assert [g is None for g in got] == [False] + [True] * 5
    _same(got, want, "count alone")
    got = _run(P, r, want=("feat",), want_moments=False)
    _same(got, want, "feat alone")


# ---- capture ---------------------------------------------------------------------------------------------------------------
def test_captured_call_replayed_back_to_back():
    P, r = sc.blobs_case(2)[0], sc.BLOB_RADIUS[2]
    want = sc.oracle_of_blobs(2)
    x = _up(P)
    lo = _up(P.min(axis=0)).reshape(1, 3)
    extent = tuple(float(v) for v in P.max(axis=0) - P.min(axis=0))
    batch = sna.PointBatch(x, None, torch.tensor([0, len(P)], dtype=torch.int64, device=_dev()), (len(P),))
    call = lambda: sna.shape_features(batch, r, lo=lo, extent=extent, max_cells=1 << 12)   # noqa: E731
    eager = _host(call())
    _same(eager, want, "eager")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        sh = call()
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    _same(_host(sh), eager, "three replays back to back: each zeroes the populations the one before left")
    with pytest.raises(_hip.HipLibraryError):
        dims = (1, 1, 1)
        ws = torch.empty(_hip.shape_ws_bytes(len(P), 1, 1) // 8, dtype=torch.int64, device=_dev())
        _hip.shape_points(x, sh.offsets, r, 3, lo.reshape(-1), dims, 1, ws, sh.count, launches=(0, 2))


# ---- the Python layer ------------------------------------------------------------------------------------------------------
def test_select_by_shape_against_the_oracle():
    tiles = [sc.blobs_case(2)[0], sc.known_shapes()["line"][0]]
    r = 1.0
    feat = sc.batch_oracle(tiles, r)[5]
    batch = _batch(tiles)
    sizes = [len(t) for t in tiles]
    with np.errstate(invalid="ignore"):
        for name, kw, keep in (("uprightness", dict(minimum=0.9), feat[:, 5] >= 0.9),
                               ("scattering", dict(maximum=0.05), feat[:, 2] <= 0.05)):
            assert 0.05 < keep.mean() < 0.95 and np.isnan(feat[:, 5]).sum() > 100
            out = sna.select_by_shape(batch, r, name, **kw)
            src = np.flatnonzero(keep)
            assert np.array_equal(out.src.cpu().numpy(), src), name
            assert np.array_equal(out.batch.pts.cpu().numpy(), np.concatenate(tiles)[src])
            assert out.batch.offsets.tolist() == [0, int(keep[:sizes[0]].sum()), int(keep.sum())]


def test_estimate_normals_and_shape_colors():
    P, r = sc.blobs_case(2)[0], sc.BLOB_RADIUS[2]
    want = sc.oracle_of_blobs(2)
    x = _up(P)
    n = sna.estimate_normals(x, r).cpu().numpy()
    _same((None, None, None, n, None, None), want, "towards None: the kernel's normals")
    view = sc.ORIGIN + np.array([3.0, -2.0, -40.0])                   # below the cloud: most normals turn over
    got = sna.estimate_normals(x, r, towards=view).cpu().numpy()
    with np.errstate(invalid="ignore"):
        away = ((view[None, :] - P) * want[3]).sum(axis=1) < 0.0
    assert away.sum() > 1000 and (~away & ~np.isnan(want[3][:, 0])).sum() > 10
    assert np.array_equal(got, np.where(away[:, None], -want[3], want[3]), equal_nan=True)
    assert np.array_equal(sna.estimate_normals(x, r, towards=_up(view)).cpu().numpy(), got, equal_nan=True)
    sh = sna.shape_features(x, r)
    rgb = sna.shape_colors(sh)
    assert rgb.dtype == torch.uint16 and tuple(rgb.shape) == (len(P), 3)
    ref = np.rint(np.nan_to_num(want[5][:, :3], nan=0.0) * 65535.0).astype(np.uint16)
    assert np.array_equal(rgb.cpu().view(torch.int16).numpy().view(np.uint16), ref) and (ref > 40000).sum() > 500
    assert np.array_equal(sh.feature("verticality").cpu().numpy(), want[5][:, 4], equal_nan=True)
    assert sh.FEATURE_NAMES == sc.FEATURE_NAMES
    with pytest.raises(ValueError):
        sh.feature("roundness")
