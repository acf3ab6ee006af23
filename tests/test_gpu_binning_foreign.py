"""K1's binning of points a grid was NOT built from, on the MI355X: the counting scatter, the LDS-bitmap kernels with
their exact fallback, and the per-point read-back (sn_gather_points), given descriptors of their own (sn_voxel_prepare on
another cloud, sn_voxel_desc_from_bounds, sn_voxel_desc_sized) and points below, above, on and one ulp around every edge,
far outside, infinite and NaN.  Everything is compared bit for bit with the rule written once in numpy fp64
(tests/binning_cases.py: np.clip(np.searchsorted(edges, p) - 1, 0, n), index n = outside); no tolerance anywhere.
Reference for the rule: pyntcloud VoxelGrid.compute as restated in oracle/voxel_oracle.py:73."""
import numpy as np
import pytest
import torch

import binning_cases as bc
import scene_net_amd as sna
from scene_net_amd import _hip
from scene_net_amd.voxelization import VoxelGrids

pytestmark = pytest.mark.gpu

_ids = lambda cases: ["-".join([k, "x".join(map(str, d))]) for k, d in cases]   # noqa: E731
N_MODE = [(k, d) for k in ("own", "bounds") for d in bc.DIMS]
BITMAP = [(k, d) for k in ("own", "bounds") for d in bc.DIMS[1:]] + [("bounds", bc.SLAB_DIMS)]
_cache = {}


def _descriptors(kind, dims, dev):
    """(device desc [4, len], host desc, own dims | None, tiles, labels): the device's tables, bit for bit the ones
    tests/binning_cases.py builds with numpy -- so the expectation and the kernels bin with the same edges -- and the
    three-tile foreign batch made for rows 0-2 of them.  Built once per (kind, dims)."""
    key = (kind, dims)
    if key in _cache:
        return _cache[key]
    host, own = bc.host_desc(kind, dims, 4)
    if kind == "bounds":
        bounds = torch.from_numpy(np.stack([bc.bounds_box(b) for b in range(4)])).to(dev)
        desc = _hip.voxel_desc(bounds, dims, from_bounds=True)
    else:
        clouds = sna.PointBatch.from_tiles([bc.own_cloud(b) for b in range(4)], device=dev)
        if kind == "own":
            desc, _ = _hip.voxel_prepare(clouds.pts, clouds.offsets, dims, regular=True)
        else:
            desc, d_dims, status = _hip.voxel_desc_sized(_hip.voxel_bbox(clouds.pts, clouds.offsets), bc.VOXEL_SIZE, dims)
            assert d_dims.cpu().tolist() == own.tolist() and status.cpu().tolist() == [0] * 4
    assert np.array_equal(desc.cpu().numpy(), host), "the device's edge tables differ from numpy's"
    tiles, labels = bc.foreign_batch(host, dims, own)
    _cache[key] = (desc, host, own, tiles, labels)
    return _cache[key]


def _batch(tiles, labels, dev, aligned=True):
    """PointBatch of tiles (an empty one allowed) on a 16-byte aligned buffer, or on the 8-byte-offset view of
    test_unaligned_point_buffer."""
    pts = np.concatenate(tiles)
    n = len(pts)
    if aligned:
        d_pts = torch.from_numpy(pts).to(dev)
        assert d_pts.data_ptr() % 16 == 0
    else:
        big = torch.zeros(n * 3 + 1, dtype=torch.float64, device=dev)
        d_pts = big[1:].view(n, 3)
        d_pts.copy_(torch.from_numpy(pts))
        assert d_pts.data_ptr() % 16 == 8
    lab = None if labels is None else torch.from_numpy(np.concatenate(labels)).to(dev)
    sizes = tuple(len(t) for t in tiles)
    offsets = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int64, device=dev)
    return sna.PointBatch(d_pts, lab, offsets, sizes)


# ------------------------------------------------------------------ read-back
GATHER = N_MODE + [("sized", bc.CAPACITY)]


@pytest.mark.parametrize("kind,dims", GATHER, ids=_ids(GATHER))
def test_gather_points_foreign(hip_device, kind, dims):
    """sn_gather_points over descriptors (a) own box of another cloud, (b) caller-given bounds, (c) size mode; f32 and f64;
    C in {1, 3}; fill in {0, -7.5, NaN}; aligned and 8-byte-offset point buffers; four tiles of 1001, 1, 0 and 2 + n points.
    The grid is arange over [B, C, nz, nx, ny]: every cell is unique (and exact in f32, < 2^24), so a point that reads another
    tile's grid, another channel or another cell shows.  (c): a point beyond the tile's OWN last edge gets `fill`, not
    the padding cell the +inf edges would give it."""
    desc, host, own, tiles, _ = _descriptors(kind, dims, hip_device)
    nx, ny, nz = dims
    order = [0, 1, 3, 2]                                  # the empty tile is third: the last tile reads grid 3 with ITS table
    tiles4 = [tiles[0], tiles[1], np.empty((0, 3)), tiles[2]]
    desc4, host4 = desc[order].contiguous(), host[order]
    own4 = None if own is None else own[order]
    if own is not None:
        b = 3
        beyond = (bc.expected_flat(host4[b], dims, tiles4[b]) >= 0) & (bc.expected_flat(host4[b], dims, tiles4[b], own4[b]) < 0)
        assert beyond.sum() > 100                         # finite and infinite points above the tile's own last edges
    assert nx * ny * nz * 4 * 3 < 2 ** 24
    for aligned in (True, False):
        batch = _batch(tiles4, None, hip_device, aligned)
        for dt in (torch.float32, torch.float64):
            for C in (1, 3):
                grid = torch.arange(4 * C * nz * nx * ny, dtype=dt, device=hip_device).reshape(4, C, nz, nx, ny)
                grid_h = grid.cpu().numpy()
                for fill in (0.0, -7.5, float("nan")):
                    got = _hip.gather_points(grid, batch.pts, batch.offsets, desc4, fill).cpu().numpy()
                    want = bc.expected_gather(grid_h, host4, dims, tiles4, fill, own4)
                    assert got.shape == want.shape and got.dtype == want.dtype
                    assert np.array_equal(got, want, equal_nan=True), (aligned, dt, C, fill)


def test_point_predictions_fill_and_tau(hip_device):
    """point_predictions(.., fill=, tau=): a dropped point's label is `fill >= tau`; a NaN fill gives 0."""
    dims = (16, 32, 8)
    desc, host, _, tiles, labels = _descriptors("bounds", dims, hip_device)
    batch = _batch(tiles, labels, hip_device)
    bounds = torch.from_numpy(np.stack([bc.bounds_box(b) for b in range(3)])).to(hip_device)
    grids = sna.voxelize_batch(batch, dims, bounds=bounds, want_counts=True)
    assert torch.equal(grids.desc, desc[:3])
    pred = torch.rand((3, 2, 8, 16, 32), device=hip_device)
    outside = np.concatenate([bc.expected_flat(host[b], dims, tiles[b]) < 0 for b in range(3)])
    assert 0.2 < outside.mean() < 0.8
    for fill in (0.0, 0.7, float("nan")):
        want = bc.expected_gather(pred.cpu().numpy(), host, dims, tiles, fill)
        got = sna.point_predictions(pred, batch, grids, fill=fill)
        assert np.array_equal(got.cpu().numpy(), want, equal_nan=True)
        for tau in (0.5, 0.9):
            lab = sna.point_predictions(pred, batch, grids, fill=fill, tau=tau).cpu().numpy()
            assert lab.dtype == np.float32 and np.array_equal(lab, (want >= tau).astype(np.float32))
            assert (lab[:, outside] == (1.0 if fill >= tau else 0.0)).all()


def test_point_predictions_on_a_point_buffer_longer_than_the_batch(hip_device):
    """the kernel strides `out`'s channels by offsets[B]; a PointBatch whose point buffer is longer than the batch (a ring
    slot) must still give [C, total_points] with every channel in its place"""
    dims = (8, 12, 4)
    desc, host, _, tiles, _ = _descriptors("own", dims, hip_device)
    exact = _batch(tiles, None, hip_device)
    n = exact.total_points
    slot = torch.full((n + 777, 3), float("nan"), dtype=torch.float64, device=hip_device)
    slot[:n] = exact.pts
    batch = sna.PointBatch(slot, None, exact.offsets, exact.sizes)
    grids = VoxelGrids(None, None, None, None, None, None, desc[:3].contiguous(), None)
    pred = torch.arange(3 * 2 * 4 * 8 * 12, dtype=torch.float64, device=hip_device).reshape(3, 2, 4, 8, 12)
    got = sna.point_predictions(pred, batch, grids, fill=-1.0).cpu().numpy()
    want = bc.expected_gather(pred.cpu().numpy(), host, dims, tiles, -1.0)
    assert got.shape == (2, n)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_gather_points_refuses_mismatched_shapes_before_launching(hip_device):
    """host-side shape checks (no synchronisation): a desc that is not [B, desc_len(nx, ny, nz)] -- a short one would be
    read out of bounds --, offsets.numel() != B + 1, pts not [N, 3]"""
    dims = (8, 12, 4)
    desc, _, _, tiles, _ = _descriptors("own", dims, hip_device)
    batch = _batch(tiles, None, hip_device)
    grid = torch.zeros((3, 1, 4, 8, 12), device=hip_device)
    d3 = desc[:3].contiguous()
    assert _hip.gather_points(grid, batch.pts, batch.offsets, d3).shape == (1, batch.total_points)
    short = _hip.voxel_desc(torch.from_numpy(np.stack([bc.bounds_box(b) for b in range(3)])).to(hip_device), (4, 12, 4),
                            from_bounds=True)
    for bad in (short, desc, d3[:2].contiguous(), d3.reshape(-1)):
        with pytest.raises(sna.HipLibraryError, match="desc must be"):
            _hip.gather_points(grid, batch.pts, batch.offsets, bad)
    for bad in (batch.offsets[:-1].contiguous(), torch.cat([batch.offsets, batch.offsets[-1:]])):
        with pytest.raises(sna.HipLibraryError, match="offsets must have"):
            _hip.gather_points(grid, batch.pts, bad, d3)
    for bad in (batch.pts.reshape(-1), batch.pts[:, :2].contiguous(), batch.pts.reshape(-1, 3, 1)):
        with pytest.raises(sna.HipLibraryError, match=r"pts must be \[N,3\]"):
            _hip.gather_points(grid, bad, batch.offsets, d3)


# ------------------------------------------------------------------ counting scatter
@pytest.mark.parametrize("kind,dims", N_MODE, ids=_ids(N_MODE))
def test_voxel_scatter_foreign(hip_device, kind, dims):
    """sn_voxel_scatter with labels and a two-entry keep list: counts, towers and dropped equal the expectation, and every
    point is either counted or dropped -- once."""
    desc, host, _, tiles, labels = _descriptors(kind, dims, hip_device)
    counts, towers, dropped = bc.expected_scatter(host, dims, tiles, labels)
    for aligned in (True, False):
        batch = _batch(tiles, labels, hip_device, aligned)
        c, t, d = _hip.voxel_scatter(batch.pts, batch.labels, batch.offsets, desc[:3].contiguous(), dims, bc.KEEP,
                                     want_towers=True)
        c, t, d = c.cpu().numpy(), t.cpu().numpy(), d.cpu().numpy()
        assert np.array_equal(d, dropped), (d, dropped)
        assert np.array_equal(c, counts) and np.array_equal(t, towers)
        assert (c.sum(axis=(1, 2, 3)) + d).tolist() == list(batch.sizes)


# ------------------------------------------------------------------ LDS bitmap
@pytest.mark.parametrize("kind,dims", BITMAP, ids=_ids(BITMAP))
def test_voxel_occupancy_foreign(hip_device, kind, dims):
    """sn_voxel_occupancy with a caller-given descriptor and foreign points, u8 and f32, with and without the tower plane,
    aligned and 8-byte-offset buffers: occ == ToFullDense(normalize_xyz(expected counts)), gt_occ == (expected towers > 0),
    dropped exact -- at (64, 128, 128) the bitmap takes two z-slabs (four with gt_occ), whose workgroups all see the dropped
    points, which are counted once."""
    assert _hip.occupancy_supported(dims, 2) and not _hip.occupancy_supported(bc.DIMS[0], 1)
    desc, host, _, tiles, labels = _descriptors(kind, dims, hip_device)
    counts, towers, dropped = bc.expected_scatter(host, dims, tiles, labels)
    occ = bc.expected_occ(counts)
    d3 = desc[:3].contiguous()
    for aligned in (True, False):
        batch = _batch(tiles, labels, hip_device, aligned)
        for dt in (torch.uint8, torch.float32):
            for want_gt in (False, True):
                o, g, flags, d = _hip.voxel_occupancy(batch.pts, batch.labels, batch.offsets, d3, dims, bc.KEEP,
                                                      want_gt_occ=want_gt, out_dtype=dt)
                assert o.dtype == dt and np.array_equal(d.cpu().numpy(), dropped), (aligned, dt, want_gt, d, dropped)
                assert np.array_equal(o[:, 0].cpu().numpy().astype(np.float64), occ), (aligned, dt, want_gt)
                assert (g is None) == (not want_gt)
                if want_gt:
                    assert np.array_equal(g[:, 0].cpu().numpy() != 0, towers > 0), (aligned, dt)


def test_voxel_occupancy_full_column_with_foreign_points(hip_device):
    """(8, 12, 4), caller-given bounds: a tile with a point in every (z, x) row -- one y column occupied in all of them --
    plus foreign points.  No row is empty, so the flag is raised (a tile's flag is up iff none of its rows is empty); with
    the exact fallback the result is the oracle's `count > column minimum`, which differs from `count > 0` here; dropped
    is exact either way."""
    dims = (8, 12, 4)
    nx, ny, nz = dims
    desc, host, _, tiles, labels = _descriptors("bounds", dims, hip_device)
    (ex, ey, ez), _ = bc.tables_of(host[0], dims)
    cx, cy, cz = [(e[:-1] + e[1:]) / 2 for e in (ex, ey, ez)]
    col = np.stack(np.meshgrid(cx, [cy[5]], cz, indexing="ij"), -1).reshape(-1, 3)     # one point per (z, x) row, y = 5
    full = np.concatenate([tiles[0], col, col[::3]])
    tiles2 = [full, tiles[1], tiles[2]]
    labels2 = [np.concatenate([labels[0], np.full(len(full) - len(labels[0]), 15.0)]), labels[1], labels[2]]
    counts, towers, dropped = bc.expected_scatter(host, dims, tiles2, labels2)
    assert counts[0, :, :, 5].min() >= 1
    want = bc.expected_occ(counts)
    assert not np.array_equal(want[0], counts[0] > 0)     # the column rule matters for this tile
    flagged = [int(v) for v in (counts.sum(axis=3) > 0).all(axis=(1, 2))]
    assert flagged[0] == 1 and flagged[1] == 0
    batch = _batch(tiles2, labels2, hip_device)
    d3 = desc[:3].contiguous()
    for dt in (torch.uint8, torch.float32):
        o, g, flags, d = _hip.voxel_occupancy(batch.pts, batch.labels, batch.offsets, d3, dims, bc.KEEP, want_gt_occ=True,
                                              out_dtype=dt, exact_fallback=True)
        assert flags.cpu().tolist() == flagged and np.array_equal(d.cpu().numpy(), dropped)
        assert np.array_equal(o[:, 0].cpu().numpy() != 0, want != 0)
        assert np.array_equal(g[:, 0].cpu().numpy() != 0, towers > 0)
        # without the fallback the flagged tile is left at `count > 0`: the flag is what tells the caller
        o2, _, flags2, d2 = _hip.voxel_occupancy(batch.pts, batch.labels, batch.offsets, d3, dims, bc.KEEP, out_dtype=dt,
                                                 exact_fallback=False)
        assert flags2.cpu().tolist() == flagged and np.array_equal(d2.cpu().numpy(), dropped)
        assert np.array_equal(o2[:, 0].cpu().numpy() != 0, counts > 0)


# ------------------------------------------------------------------ voxelize_batch(bounds=...)
BOUNDS = bc.DIMS + [bc.SLAB_DIMS]


@pytest.mark.parametrize("dims", BOUNDS, ids=["x".join(map(str, d)) for d in BOUNDS])
def test_voxelize_batch_with_bounds_foreign(hip_device, dims):
    """voxelize_batch(bounds=...) -- a fixed box shared by points it was not made from: the counting route
    (want_counts=True) and the occupancy-only route agree with each other and with the expectation, .dropped included.  At
    (5, 7, 3) the bitmap kernels do not serve the grid: the occupancy-only request must take the counting kernels."""
    desc, host, _, tiles, labels = _descriptors("bounds", dims, hip_device)
    counts, towers, dropped = bc.expected_scatter(host, dims, tiles, labels)
    occ = bc.expected_occ(counts)
    bounds = torch.from_numpy(np.stack([bc.bounds_box(b) for b in range(3)])).to(hip_device)
    for aligned in (True, False):
        batch = _batch(tiles, labels, hip_device, aligned)
        slow = sna.voxelize_batch(batch, dims, bc.KEEP, want_occ=True, want_gt_occ=True, bounds=bounds, want_counts=True)
        fast = sna.voxelize_batch(batch, dims, bc.KEEP, want_occ=True, want_gt_occ=True, bounds=bounds)
        assert slow.counts is not None and (fast.counts is None) == _hip.occupancy_supported(dims, 2)
        assert (fast.counts is None) == (dims != bc.DIMS[0])
        assert np.array_equal(slow.counts.cpu().numpy(), counts) and np.array_equal(slow.towers.cpu().numpy(), towers)
        for g in (slow, fast):
            assert torch.equal(g.desc, desc[:3])
            assert np.array_equal(g.dropped.cpu().numpy(), dropped), (aligned, g.dropped, dropped)
            assert np.array_equal(g.occ[:, 0].cpu().numpy(), occ.astype(np.float32))
            assert np.array_equal(g.gt_occ[:, 0].cpu().numpy(), (towers > 0).astype(np.float32))
        assert torch.equal(slow.occ, fast.occ) and torch.equal(slow.gt_occ, fast.gt_occ)
        assert torch.equal(slow.dropped, fast.dropped)
