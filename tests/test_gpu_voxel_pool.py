"""K24 on the GPU: sn_voxel_pool and the layers above it against the numpy restatement of tests/voxel_pool_cases.py.  Every
comparison is exact: integers as they are, fp64 as int64 views.  With and without the look before a min / max atomic; K1's
binning of foreign points with own, given and size-mode descriptors;
seams of the chunk, empty tiles, one crowded voxel, permuted rows, buffers offset by one element, sentinel-filled outputs
with guard slots, capture, and parity with sn_voxel_scatter's counts and sn_voxel_classes' grid."""
import os
import struct

import numpy as np
import pytest
import torch

import binning_cases as bc
import voxel_pool_cases as pc
import scene_net_amd as sna
from scene_net_amd import _hip

pytestmark = pytest.mark.gpu

GUARD = 5                      # sentinel slots behind every output
SENT_F = -7.25e300             # what an untouched fp64 slot holds
SENT_I = -99


def shifted(arr, dev, shift):
    """The array on the device, `shift` elements into a larger buffer (8-byte aligned, not 16)."""
    flat = torch.from_numpy(np.ascontiguousarray(arr)).reshape(-1)
    buf = torch.empty(flat.numel() + shift, dtype=flat.dtype, device=dev)
    view = buf[shift:]
    view.copy_(flat)
    return view.reshape(arr.shape)


def sentinel(n, value, dtype, dev, shift):
    return torch.full((n + GUARD + shift,), value, dtype=dtype, device=dev)[shift:]


def run_pool(dev, tiles, dims, desc, sources, ops, values=None, ranges=None, fill=0.0, shift=0, look=True):
    """One sn_voxel_pool through the ctypes layer with sentinel-filled outputs; numpy copies of everything."""
    sizes = [len(t) for t in tiles]
    B, V, P = len(tiles), dims[0] * dims[1] * dims[2], len(sources)
    pts = shifted(np.concatenate(tiles).astype(np.float64), dev, shift)
    val = None if values is None else shifted(np.concatenate(values).astype(np.float64), dev, shift)
    offsets = shifted(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64), dev, shift)
    d = shifted(np.asarray(desc, dtype=np.float64), dev, shift)
    out = sentinel(B * P * V, SENT_F, torch.float64, dev, shift)
    counts = sentinel(B * V, SENT_I, torch.int32, dev, shift)           # (4-byte aligned, not 8)
    unb = sentinel(B, SENT_I, torch.int64, dev, shift)
    nans = sentinel(B, SENT_I, torch.int64, dev, shift)
    assert _hip.voxel_pool_ws_bytes(B, dims, P) == 0                      # the accumulators live in the outputs
    _hip.voxel_pool(pts, val, offsets, d, dims, sources, ops, ranges, fill, out[:B * P * V], counts[:B * V], unb[:B], nans[:B],
                    look=look)
    torch.cuda.synchronize()
    o, c, u, n = out.cpu().numpy(), counts.cpu().numpy(), unb.cpu().numpy(), nans.cpu().numpy()
    assert np.all(o[B * P * V:] == SENT_F) and np.all(c[B * V:] == SENT_I) and np.all(u[B:] == SENT_I) and np.all(n[B:] == SENT_I), \
        "guard slots were touched"
    nx, ny, nz = dims
    return o[:B * P * V].reshape(B, P, nz, nx, ny), c[:B * V].reshape(B, nz, nx, ny), u[:B], n[:B]


def check(out, exp):
    assert np.array_equal(out[1], exp[1]), "counts"
    assert np.array_equal(out[2], exp[2]) and np.array_equal(out[3], exp[3]), "unbinned / nan_rows"
    assert np.array_equal(pc.bits(out[0]), pc.bits(exp[0])), "planes"


def check_every_way(dev, tiles, dims, desc, sources, ops, exp, shifts=(0,), **kw):
    for shift in shifts:
        check(run_pool(dev, tiles, dims, desc, sources, ops, shift=shift, **kw), exp)
    if any(op != pc.MEAN for op in ops):
        check(run_pool(dev, tiles, dims, desc, sources, ops, look=False, **kw), exp)


# ================================================================ the kernel
@pytest.mark.parametrize("kind,dims", [("own", (5, 7, 3)), ("bounds", (5, 7, 3)), ("own", (8, 12, 4)), ("bounds", (8, 12, 4)),
                                       ("own", (64, 64, 64)), ("bounds", (64, 64, 64)), ("sized", bc.CAPACITY)])
def test_pool_of_a_foreign_batch(hip_device, kind, dims):
    assert dims in bc.DIMS or dims == bc.CAPACITY
    desc, own, tiles = pc.foreign_case(kind, dims)
    assert [len(t) for t in tiles[:2]] == [1001, 1] and len(tiles) == 4       # an odd start offset, a one-point tile
    rng = np.random.default_rng(241)
    values = [pc.special_values(len(t), rng)[:, None] for t in tiles]
    # the centroids: no value column is read, so no row is a NaN row
    exp = pc.expected_pool(desc, dims, tiles, *pc.CENTROIDS)
    assert exp[1][3].sum() == 0 and exp[2][3] == len(tiles[3]) and exp[3].sum() == 0       # the tile with nothing binned
    assert exp[1].sum() > 1000 and exp[2].sum() > (100 if kind != "sized" else 5)
    if kind == "sized":            # the padded table is used as it stands: rows above a tile's own last edge are binned
        inside_own = sum(int((bc.expected_flat(desc[b], dims, t, own[b]) >= 0).sum()) for b, t in enumerate(tiles))
        assert exp[1].sum() > inside_own
    check_every_way(hip_device, tiles, dims, desc, *pc.CENTROIDS, exp, shifts=(0, 1))
    check(run_pool(hip_device, tiles, dims, desc, *pc.CENTROIDS, values=values), exp)       # values given, not read
    # eight planes: mean, min and max of z and of a column of NaN, +-inf, +-0.0, denormals and ordinary numbers
    exp8 = pc.expected_pool(desc, dims, tiles, *pc.EIGHT, values=values, ranges=[pc.VALUE_RANGE], fill=-2.5)
    assert exp8[3].sum() > 50 and np.isinf(exp8[0]).any() and (exp8[0] == -2.5).any()
    assert np.array_equal(exp8[1].sum(axis=(1, 2, 3)) + exp8[2] + exp8[3], [len(t) for t in tiles])
    check_every_way(hip_device, tiles, dims, desc, *pc.EIGHT, exp8, shifts=(0, 1), values=values, ranges=[pc.VALUE_RANGE],
                    fill=-2.5)


def test_totals_and_tile_borders_on_the_chunk_seams(hip_device):
    c = _hip.voxel_pool_chunk_points()
    dims = (5, 7, 3)
    rng = np.random.default_rng(242)
    src, ops = [2, 3, 3, 0], [pc.MEAN, pc.MEAN, pc.MAX, pc.MIN]
    cloud = pc.cube_tile(50, 9)
    for total in (c - 1, c, c + 1):
        # one tile; then borders inside the chunk, on the seam and an empty tile on either side of it
        for sizes in ([total], [7, total - 7], [c - 1, 0, total - (c - 1)], [total - 1, 0, 1]):
            sizes = [n for n in sizes if n >= 0]
            assert sum(sizes) == total
            tiles = [pc.cube_tile(n, 11 + k + total) if n else np.empty((0, 3)) for k, n in enumerate(sizes)]
            desc = np.stack([pc.own_desc(t if len(t) else cloud, dims) for t in tiles])
            values = [pc.special_values(len(t), rng)[:, None] for t in tiles]
            exp = pc.expected_pool(desc, dims, tiles, src, ops, values=values, ranges=[pc.VALUE_RANGE])
            assert exp[2].sum() == 0
            check_every_way(hip_device, tiles, dims, desc, src, ops, exp, values=values, ranges=[pc.VALUE_RANGE])
    sizes = [c - 1, 1, 1, c + 2, 3]
    tiles = [pc.cube_tile(n, 90 + k) for k, n in enumerate(sizes)]
    desc = np.stack([pc.own_desc(t, dims) for t in tiles])
    check_every_way(hip_device, tiles, dims, desc, *pc.CENTROIDS, pc.expected_pool(desc, dims, tiles, *pc.CENTROIDS))


def test_rows_behind_the_last_offset_are_not_read(hip_device):
    dims = (5, 7, 3)
    tile = pc.cube_tile(300, 21)
    desc = pc.own_desc(tile, dims)[None]
    exp = pc.expected_pool(desc, dims, [tile], *pc.CENTROIDS)
    packed = torch.from_numpy(np.concatenate([tile, np.full((9, 3), np.nan)])).to(hip_device)
    offsets = torch.tensor([0, 300], dtype=torch.int64, device=hip_device)
    out = torch.empty((1, 3, 3, 5, 7), dtype=torch.float64, device=hip_device)
    counts = torch.empty((1, 3, 5, 7), dtype=torch.int32, device=hip_device)
    unb, nans = (torch.empty((1,), dtype=torch.int64, device=hip_device) for _ in range(2))
    _hip.voxel_pool(packed, None, offsets, torch.from_numpy(desc).to(hip_device), dims, *pc.CENTROIDS, None, 0.0, out, counts,
                    unb, nans)
    check((out.cpu().numpy(), counts.cpu().numpy(), unb.cpu().numpy(), nans.cpu().numpy()), exp)


def crowded_tile(dims, rng):
    """4097 rows of one tile in one cell, about 600 spread over the rest; shuffled"""
    base = pc.cube_tile(600, 31)
    desc = pc.own_desc(base, dims)[None]
    lo, hi = desc[0, :3], desc[0, 3:6]
    step = (hi - lo) / np.array(dims)
    crowd = lo + step * np.array([2.5, 3.5, 1.5]) + (rng.random((4097, 3)) - 0.5) * 0.8 * step
    f_crowd = int(bc.expected_flat(desc[0], dims, crowd)[0])
    tile = np.concatenate([base[bc.expected_flat(desc[0], dims, base) != f_crowd], crowd])
    tile = tile[rng.permutation(len(tile))]
    assert (bc.expected_flat(desc[0], dims, tile) == f_crowd).sum() == 4097
    return tile, desc, f_crowd


def test_one_crowded_voxel_and_permuted_rows(hip_device):
    dims = (5, 7, 3)
    rng = np.random.default_rng(243)
    tile, desc, f_crowd = crowded_tile(dims, rng)
    values = pc.special_values(len(tile), rng, nan_share=0.02)[:, None]
    exp = pc.expected_pool(desc, dims, [tile], *pc.EIGHT, values=[values], ranges=[pc.VALUE_RANGE])
    in_crowd = bc.expected_flat(desc[0], dims, tile) == f_crowd
    assert exp[1].reshape(-1)[f_crowd] == 4097 - np.isnan(values[in_crowd, 0]).sum() > 3000      # (NaN rows take no part)
    check_every_way(hip_device, [tile], dims, desc, *pc.EIGHT, exp, values=[values], ranges=[pc.VALUE_RANGE])
    # ascending and descending values: every row of the crowd moves the cell, or only the first does
    for direction in (1, -1):
        v = np.arange(len(tile), dtype=np.float64)[::direction].copy()[:, None]
        e = pc.expected_pool(desc, dims, [tile], [3, 3], [pc.MIN, pc.MAX], values=[v])
        check_every_way(hip_device, [tile], dims, desc, [3, 3], [pc.MIN, pc.MAX], e, values=[v])
    # the same tile with its rows permuted: the same bits
    for seed in (1, 2):
        order = np.random.default_rng(seed).permutation(len(tile))
        check(run_pool(hip_device, [tile[order]], dims, desc, *pc.EIGHT, values=[values[order]], ranges=[pc.VALUE_RANGE]), exp)


def test_counts_are_the_scatter_kernels_and_a_max_plane_is_the_class_grid(hip_device):
    dims = (8, 12, 4)
    desc, _, tiles = pc.foreign_case("own", dims)
    rng = np.random.default_rng(244)
    labels = [bc.LABELS[rng.integers(0, len(bc.LABELS), len(t))] for t in tiles]          # finite labels
    batch = sna.PointBatch.from_tiles(tiles, labels, device=hip_device)
    d = torch.from_numpy(desc).to(hip_device)
    ref_counts, _, dropped = _hip.voxel_scatter(batch.pts, None, batch.offsets, d, dims)
    B = len(tiles)
    grid = torch.empty((B, 1, 4, 8, 12), dtype=torch.float64, device=hip_device)
    unb, nans = (torch.empty((B,), dtype=torch.int64, device=hip_device) for _ in range(2))
    _hip.voxel_classes(batch.pts, batch.labels, batch.offsets, d, dims, grid, unb, nans)
    vp = sna.voxel_pool(batch, dims, ("x.mean", "y.mean", "z.mean"), desc=d)
    assert vp.counts.dtype == torch.int32 and torch.equal(vp.counts, ref_counts)
    assert torch.equal(vp.unbinned, dropped.to(torch.int64)) and int(vp.nan_rows.sum()) == 0
    top = sna.voxel_pool(batch, dims, ("v0.max",), values=batch.labels, desc=d, fill=0.0)
    assert torch.equal(top.planes.view(torch.int64), grid.view(torch.int64)) and torch.equal(top.unbinned, unb)
    assert torch.equal(top.counts, ref_counts)


def test_one_plane_two_planes_of_one_source_and_a_nan_fill(hip_device):
    dims = (8, 12, 4)
    tiles = [pc.cube_tile(1301, 41), pc.cube_tile(5, 42)]
    desc = np.stack([pc.own_desc(t, dims) for t in tiles])
    nan_bits = 0x7FF8000000012345
    fill = struct.unpack("<d", struct.pack("<Q", nan_bits))[0]
    for src, ops in (([1], [pc.MEAN]), ([2], [pc.MAX]), ([0, 0], [pc.MEAN, pc.MEAN]), ([2, 2], [pc.MIN, pc.MIN])):
        exp = pc.expected_pool(desc, dims, tiles, src, ops, fill=fill)
        empty = exp[1] == 0
        assert empty.any() and (pc.bits(exp[0])[:, 0][empty] == nan_bits).all()
        out = run_pool(hip_device, tiles, dims, desc, src, ops, fill=fill)
        check(out, exp)
        if len(src) == 2:
            assert np.array_equal(pc.bits(out[0][:, 0]), pc.bits(out[0][:, 1]))
    neg_zero = run_pool(hip_device, tiles, dims, desc, [0], [pc.MEAN], fill=-0.0)
    assert (pc.bits(neg_zero[0])[:, 0][neg_zero[1] == 0] == np.int64(-2 ** 63)).all()


def test_captured_call_replayed_with_new_input(hip_device, monkeypatch):
    dims = (8, 12, 4)
    rng = np.random.default_rng(245)
    n = [1500, 900]
    tiles = [pc.cube_tile(n[0], 51), pc.cube_tile(n[1], 52)]
    desc = np.stack([pc.own_desc(t, dims) for t in tiles])
    inputs = []
    for k in range(2):
        moved = [t + (rng.random(t.shape) - 0.5) * (3.0 * k) for t in tiles]         # (k = 1: some rows leave their table)
        inputs.append((np.concatenate(moved), np.concatenate([pc.special_values(m, rng) for m in n])[:, None]))
    pts = torch.from_numpy(inputs[0][0]).to(hip_device)
    val = torch.from_numpy(inputs[0][1]).to(hip_device)
    offsets = torch.tensor([0, n[0], sum(n)], dtype=torch.int64, device=hip_device)
    d = torch.from_numpy(desc).to(hip_device)
    src, ops = pc.EIGHT
    out = torch.empty((2, 8, 4, 8, 12), dtype=torch.float64, device=hip_device)
    counts = torch.empty((2, 4, 8, 12), dtype=torch.int32, device=hip_device)
    unb, nans = (torch.empty((2,), dtype=torch.int64, device=hip_device) for _ in range(2))
    outs = [out, counts, unb, nans]

    def launch():
        _hip.voxel_pool(pts, val, offsets, d, dims, src, ops, [pc.VALUE_RANGE], 0.0, out, counts, unb, nans)

    def load(k):
        pts.copy_(torch.from_numpy(inputs[k][0]))
        val.copy_(torch.from_numpy(inputs[k][1]))
        for t in outs:
            t.view(torch.uint8).fill_(0x5a)

    load(0)
    launch()                                                 # (eager first: the kernels are loaded)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch()
    seen = []
    for k in (0, 1, 0):
        load(k)
        graph.replay()
        torch.cuda.synchronize()
        got = [t.cpu().numpy().copy() for t in outs]
        split = [inputs[k][0][:n[0]], inputs[k][0][n[0]:]], [inputs[k][1][:n[0]], inputs[k][1][n[0]:]]
        exp = pc.expected_pool(desc, dims, split[0], src, ops, values=split[1], ranges=[pc.VALUE_RANGE])
        check(got, exp)
        seen.append(got[0].tobytes())
    assert seen[0] == seen[2] and seen[0] != seen[1]
    del graph
    # ranges taken on the device are a host read: refused while the stream captures
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(sna.HipLibraryError, match="value_ranges"):
        sna.voxel_pool(sna.PointBatch(pts, None, offsets, tuple(n)), dims, ("v0.mean",), values=val, desc=d)


# ================================================================ the layers
def test_voxel_pool_layer_names_ranges_and_round_trip(hip_device):
    dims = (8, 12, 4)
    rng = np.random.default_rng(246)
    tiles = [pc.cube_tile(1301, 41), pc.cube_tile(5, 42), pc.cube_tile(700, 43, extent=31.0)]
    batch = sna.PointBatch.from_tiles(tiles, device=hip_device)
    host = np.stack([pc.own_desc(t, dims) for t in tiles])
    cen = sna.voxel_centroids(batch, dims)
    assert tuple(cen.planes.shape) == (3, 3, 4, 8, 12) and cen.planes.dtype == torch.float64 and cen.dims is None
    assert cen.names == ("x.mean", "y.mean", "z.mean")
    assert np.array_equal(pc.bits(cen.desc.cpu().numpy()), pc.bits(host))        # the grid both sides bin with
    exp = pc.expected_pool(host, dims, tiles, *pc.CENTROIDS)
    check((cen.planes.cpu().numpy(), cen.counts.cpu().numpy(), cen.unbinned.cpu().numpy(), cen.nan_rows.cpu().numpy()), exp)
    # every point gets its voxel's centroid: it lies in the point's own voxel, so no further away than a voxel's diagonal
    back = _hip.gather_points(cen.planes, batch.pts, batch.offsets, cen.desc).cpu().numpy()
    flat = np.concatenate([bc.expected_flat(host[b], dims, t) + b * 384 for b, t in enumerate(tiles)])
    want = np.stack([cen.planes.cpu().numpy()[:, a].reshape(-1)[flat] for a in range(3)])
    assert np.array_equal(pc.bits(back), pc.bits(want))
    # value columns by name; ranges taken on the device are the columns' finite extrema
    feat = np.stack([rng.random(batch.total_points), pc.special_values(batch.total_points, rng)], axis=1)
    fv = torch.from_numpy(feat).to(hip_device)
    names = ("v0.mean", "v1.mean", "v1.max", "z.min")
    vp = sna.voxel_pool(batch, dims, names, values=fv, fill=-1.0)
    fin = feat[np.isfinite(feat[:, 1]), 1]
    ranges = [(feat[:, 0].min(), feat[:, 0].max()), (fin.min(), fin.max())]
    split = np.split(feat, np.cumsum([len(t) for t in tiles])[:-1])
    e = pc.expected_pool(host, dims, tiles, [3, 4, 4, 2], [pc.MEAN, pc.MEAN, pc.MAX, pc.MIN], values=split, ranges=ranges, fill=-1.0)
    check((vp.planes.cpu().numpy(), vp.counts.cpu().numpy(), vp.unbinned.cpu().numpy(), vp.nan_rows.cpu().numpy()), e)
    assert vp.names == names and int(vp.nan_rows.sum()) > 50
    given = sna.voxel_pool(batch, dims, names, values=fv, value_ranges=ranges, fill=-1.0)
    assert torch.equal(given.planes.view(torch.int64), vp.planes.view(torch.int64))
    # size mode: the descriptor voxelize_batch builds for the same arguments
    sized = sna.voxel_pool(batch, bc.CAPACITY, voxel_dims=bc.VOXEL_SIZE)
    ref = sna.voxelize_batch(batch, bc.CAPACITY, voxel_dims=bc.VOXEL_SIZE, want_density=True, want_occ=False)
    assert torch.equal(sized.desc.view(torch.int64), ref.desc.view(torch.int64)) and torch.equal(sized.dims, ref.dims)
    assert torch.equal(sized.counts, ref.counts)
    se = pc.expected_pool(sized.desc.cpu().numpy(), bc.CAPACITY, tiles, *pc.CENTROIDS)
    check((sized.planes.cpu().numpy(), sized.counts.cpu().numpy(), sized.unbinned.cpu().numpy(), sized.nan_rows.cpu().numpy()), se)


@pytest.mark.parametrize("mode", ["n", "size"])
def test_centroid_grids_next_to_density_and_ratio(hip_device, golden_dir, mode):
    a = np.load(os.path.join(golden_dir, "ts40k_sample575_subset.npy"))
    xyz, lab = a[:, :3], a[:, 3]
    kw = dict(voxelgrid_dims=(16, 24, 8)) if mode == "n" else dict(voxelgrid_dims=(64, 64, 64), voxel_dims=(2.5, 3.0, 2.0))
    hist = sna.centroid_hist_on_voxel(xyz, **kw)
    reg = sna.centroid_reg_on_voxel(xyz, lab, bc.KEEP, **kw)
    dens = sna.hist_on_voxel(xyz, **kw)
    ratio = sna.reg_on_voxel(xyz, lab, bc.KEEP, **kw)
    assert isinstance(hist, np.ndarray) and hist.dtype == np.float64 and hist.shape == (4,) + dens.shape == reg.shape
    if mode == "n":
        assert dens.shape == (8, 16, 24)
    else:
        assert max(dens.shape) < 64                                              # cut to the tile's own dims
    assert np.array_equal(hist[:-1], reg[:-1])                                   # the reference's own assertion
    assert np.array_equal(pc.bits(hist[:-1]), pc.bits(reg[:-1]))
    assert np.array_equal(pc.bits(hist[-1]), pc.bits(dens)) and np.array_equal(pc.bits(reg[-1]), pc.bits(ratio))
    # the centroids are the restatement's on the table the density was binned with; empty voxels are 0
    batch = sna.PointBatch.from_tiles([xyz], device=hip_device)
    if mode == "n":
        table = (16, 24, 8)
        desc = pc.own_desc(xyz, table)[None]
    else:
        table = (64, 64, 64)
        desc = sna.voxelize_batch(batch, table, voxel_dims=kw["voxel_dims"], want_density=True, want_occ=False).desc.cpu().numpy()
    exp = pc.expected_pool(desc, table, [xyz], *pc.CENTROIDS)
    nz, nx, ny = dens.shape
    assert exp[1][0, :nz, :nx, :ny].sum() == len(xyz) and exp[2][0] == 0
    assert np.array_equal(pc.bits(hist[:-1]), pc.bits(exp[0][0][:, :nz, :nx, :ny]))
    assert ((hist[:-1] == 0).all(axis=0) == (exp[1][0, :nz, :nx, :ny] == 0)).all() and ((dens > 0) <= (hist[0] != 0)).all()
    lo, hi = xyz.min(axis=0), xyz.max(axis=0)
    occupied = hist[0] != 0
    assert all((hist[k][occupied] >= lo[k] - 1e-6).all() and (hist[k][occupied] <= hi[k] + 1e-6).all() for k in range(3))


def test_xyz_voxelization_on_the_ts40k_sample(hip_device, golden_dir):
    a = np.load(os.path.join(golden_dir, "ts40k_sample575_subset.npy"))
    sample = (a[:, :3], a[:, 3])
    xyz, dens, gt = sna.xyz_Voxelization(bc.KEEP, vxg_size=(16, 24, 8))(sample)
    assert xyz.shape == (1, 3, 8, 16, 24) and dens.shape == (1, 8, 16, 24) and gt.shape == (1, 8, 16, 24)
    assert all(isinstance(t, np.ndarray) and t.dtype == np.float64 for t in (xyz, dens, gt))
    hist = sna.centroid_hist_on_voxel(sample[0], (16, 24, 8))
    assert np.array_equal(pc.bits(xyz[0]), pc.bits(hist[:-1])) and np.array_equal(pc.bits(dens[0]), pc.bits(hist[-1]))
    assert np.array_equal(pc.bits(gt[0]), pc.bits(sna.reg_on_voxel(sample[0], sample[1], bc.KEEP, (16, 24, 8))))
    # the reference's Compose([xyz_Voxelization, ToTensor, xyz_ToFullDense]) chain; vox_size takes priority over vxg_size
    t = sna.xyz_ToFullDense()(sna.ToTensor()((xyz, dens, gt)))
    assert torch.equal(t[0], torch.from_numpy(xyz)) and set(np.unique(t[1].numpy())) == {0.0, 1.0}
    assert torch.equal(t[2], torch.from_numpy((gt > 0).astype(np.float64)))
    sx, sd, sg = sna.xyz_Voxelization(bc.KEEP, vox_size=(2.5, 3.0, 2.0), vxg_size=(64, 64, 64))(sample)
    assert sx.shape[:2] == (1, 3) and sx.shape[2:] == sd.shape[1:] == sg.shape[1:] and max(sd.shape) < 64


def test_voxel_downsample_against_the_restatement(hip_device):
    dims = (8, 12, 4)
    desc, _, tiles = pc.foreign_case("own", dims)
    rng = np.random.default_rng(247)
    labels = [np.where(rng.random(len(t)) < 0.2, np.nan, rng.integers(0, 20, len(t)).astype(np.float64)) for t in tiles]
    batch = sna.PointBatch.from_tiles(tiles, labels, device=hip_device)
    d = torch.from_numpy(desc).to(hip_device)
    exp = pc.expected_pool(desc, dims, tiles, *pc.CENTROIDS)
    cnt = exp[1].reshape(len(tiles), -1)
    sizes = tuple(int((c > 0).sum()) for c in cnt)
    assert sizes[1] == 0 and sizes[3] == 0 and sizes[0] > 100                    # two tiles come back empty
    rows = np.concatenate([exp[0][b].reshape(3, -1)[:, cnt[b] > 0].T for b in range(len(tiles))])
    import voxel_classes_cases as kc
    top = kc.expected_grid(desc, dims, tiles, labels)[0].reshape(len(tiles), -1)
    for rule in (None, "max"):
        small, n = sna.voxel_downsample(batch, dims, desc=d, label_rule=rule)
        assert isinstance(small, sna.PointBatch) and small.sizes == sizes
        assert np.array_equal(small.offsets.cpu().numpy(), np.concatenate([[0], np.cumsum(sizes)]))
        assert np.array_equal(pc.bits(small.pts.cpu().numpy()), pc.bits(rows))   # rows and their order
        assert n.dtype == torch.int32 and np.array_equal(n.cpu().numpy(), np.concatenate([c[c > 0] for c in cnt]))
        if rule is None:
            assert small.labels is None
        else:
            want = np.concatenate([top[b][cnt[b] > 0] for b in range(len(tiles))])
            assert np.isnan(want).any() and np.array_equal(pc.bits(small.labels.cpu().numpy()), pc.bits(want))
    own = sna.voxel_downsample(sna.PointBatch.from_tiles(tiles[:1], device=hip_device), dims)[0]
    assert own.total_points == int((pc.expected_pool(pc.own_desc(tiles[0], dims)[None], dims, tiles[:1], *pc.CENTROIDS)[1] > 0).sum())
