"""Voxel clouds (K16) on the device: sn_voxel_cloud_count / sn_voxel_cloud_scatter and their Python layer, byte for byte
against the reference's recorded rows (tests/golden/voxel_cloud.npz) and the numpy restatement (voxel_cloud_cases.py)."""
import os

import numpy as np
import pytest
import torch

import scene_net_amd as sna
from scene_net_amd import _hip

import voxel_cloud_cases as vc

pytestmark = pytest.mark.gpu

_TORCH = {"f32": torch.float32, "f64": torch.float64, "u8": torch.uint8, "bool": torch.bool}


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _same(got, want):
    """byte for byte; rows that hold a NaN are compared as values (a NaN's payload is not part of the contract)"""
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape)
    if np.isnan(want).any():
        return np.array_equal(got, want, equal_nan=True)
    return got.tobytes() == want.tobytes()


def _table(mode, r):
    return vc.jet_table(r) if mode == "ranges" else None


# ---- 1. the reference's own rows -------------------------------------------------------------------------------------------------
def test_golden_rows_byte_for_byte(hip_device, golden_dir):
    g = np.load(os.path.join(golden_dir, "voxel_cloud.npz"))
    for name, mode, r in zip(g["names"], g["modes"], g["rs"]):
        name, mode, r = str(name), str(mode), int(r)
        grid, want = g[name + "_grid"], g[name + "_rows"]
        for as_device in (False, True):
            arg = _dev(grid, hip_device) if as_device else grid
            got = sna.plot_voxelgrid(arg, mode, plot=False, r=r, color_ranges=g[f"jet_{r}"])
            if g[name + "_none"][0]:
                assert got is None, name
            else:
                assert isinstance(got, np.ndarray) and _same(got, want), name
    # one batched call over grids of one shape gives the same clouds
    same = [str(n) for n in g["names"] if g[str(n) + "_grid"].shape == (3, 4, 5) and g[str(n) + "_grid"].dtype == np.float64]
    assert len(same) >= 2
    cloud = sna.voxel_cloud(_dev(np.stack([g[n + "_grid"] for n in same]), hip_device), "density")
    assert cloud.sizes() == tuple(0 for _ in same) and cloud.rows.shape == (0, 6)


def test_default_table_is_the_embedded_jet(hip_device, golden_dir):
    g = np.load(os.path.join(golden_dir, "voxel_cloud.npz"))
    got = sna.plot_voxelgrid(g["ranges_r10_f64_grid"], "ranges", plot=False)
    assert _same(got, g["ranges_r10_f64_rows"])
    t = sna.plot_voxelgrid(_dev(g["ranges_r10_f32_grid"], hip_device), "ranges", plot=False, as_tensor=True)
    assert t.is_cuda and _same(t, g["ranges_r10_f32_rows"])


# ---- 2. chunk seams, every dtype -------------------------------------------------------------------------------------------------
def _seam_shapes():
    c = _hip.voxel_cloud_chunk_cells()
    assert c == 1024, "the shapes below put their sizes on the seams of a 1024-cell chunk"
    return [(16, 8, 8), (1, 31, 33), (1, 25, 41), (7, 1, 293), (13, 11, 9)]    # c, c - 1, c + 1, 2c + 3, 1287


@pytest.mark.parametrize("mode", vc.MODES)
def test_chunk_seams_in_every_dtype(hip_device, mode):
    sizes = [int(np.prod(s)) for s in _seam_shapes()]
    assert sizes == [1024, 1023, 1025, 2051, 1287]
    for k, shape in enumerate(_seam_shapes()):
        for tag, grid in vc.torch_dtype_grids(shape, seed=7 + k).items():
            want = vc.restate(grid, mode, 10, _table(mode, 10))
            cloud = sna.voxel_cloud(_dev(grid, hip_device).to(_TORCH[tag])[None], mode)
            assert want is not None and len(want) > 0
            assert cloud.offsets.cpu().tolist() == [0, len(want)], (shape, tag)
            assert _same(cloud.rows, want), (shape, tag)
            assert tuple(cloud.bad[0].cpu().tolist()) == vc.bad_counts(grid, mode), (shape, tag)


def test_prefix_carries_into_the_second_scan_tile(hip_device):
    """The prefix kernel scans a tile's row in tiles of 256 threads x 8 slots = 2048 chunks and carries the running total
    from one tile to the next: a grid of 2064 chunks with live cells on both sides of cell 2048 * 1024."""
    c = _hip.voxel_cloud_chunk_cells()
    shape, seam = (129, 128, 128), 256 * 8 * c       # kScanThreads * kScanItems of scan.h
    n = int(np.prod(shape))
    assert seam + 15 * c < n
    rng = np.random.default_rng(2064)
    v = rng.uniform(-1.2, 1.6, n).astype(np.float32)
    v[rng.random(n) >= 0.01] = 0.0
    v[[seam - 1, seam, n - 1]] = [0.5, -0.25, 1.0]
    grid = v.reshape(shape)
    want = vc.restate(grid, "density")
    flat = np.flatnonzero(v)
    assert 0.008 * n < len(want) < 0.012 * n and (flat < seam).sum() > 10000 and (flat >= seam).sum() > 100
    cloud = sna.voxel_cloud(_dev(grid, hip_device)[None], "density")
    assert cloud.offsets.cpu().tolist() == [0, len(want)]
    assert _same(cloud.rows, want)
    assert tuple(cloud.bad[0].cpu().tolist()) == vc.bad_counts(grid, "density")


def test_more_tiles_than_the_offsets_kernel_has_threads(hip_device):
    """257 tiles: the one workgroup of the offsets kernel (256 threads) takes a second step and carries its total"""
    shape, B = (3, 4, 5), 257
    grids = np.stack([vc.seam_grid(shape, 10, np.float64, seed=300 + b) for b in range(B)])
    grids[100] = 0.0                                 # an empty tile on the way
    want = [vc.restate(g, "density") for g in grids]
    sizes = [0 if w is None else len(w) for w in want]
    assert sizes[256] > 0 and sum(sizes[:256]) > 256 * 20
    cloud = sna.voxel_cloud(_dev(grids, hip_device), "density")
    assert cloud.offsets.cpu().tolist() == np.concatenate([[0], np.cumsum(sizes)]).tolist()
    assert _same(cloud.rows, np.concatenate([w for w in want if w is not None]))
    assert cloud.bad.cpu().tolist() == [list(vc.bad_counts(g, "density")) for g in grids]


def test_batch_with_an_empty_tile_in_the_middle(hip_device):
    shape = (13, 11, 9)
    first = vc.seam_grid(shape, 10, np.float64, seed=3)
    grids = np.stack([first, np.zeros(shape), np.full(shape, 0.625)])
    for mode in vc.MODES:
        want = [vc.restate(g, mode, 10, _table(mode, 10)) for g in grids]
        assert want[1] is None and len(want[2]) == 1287
        for grids_d in (_dev(grids, hip_device), _dev(grids, hip_device)[:, None]):      # [B,nz,nx,ny] and [B,1,nz,nx,ny]
            cloud = sna.voxel_cloud(grids_d, mode)
            assert cloud.sizes() == (len(want[0]), 0, 1287) and cloud.B == 3
            assert _same(cloud.tile(0), want[0]) and cloud.tile(1).shape == (0, 6) and _same(cloud.tile(2), want[2])


# ---- 3. capacity -----------------------------------------------------------------------------------------------------------------
def test_capacity_smaller_than_the_total(hip_device):
    shape = (13, 11, 9)
    grids = np.stack([vc.seam_grid(shape, 10, np.float64, seed=s) for s in (11, 12)])
    want = np.concatenate([vc.restate(g, "density") for g in grids])
    sizes = [len(vc.restate(g, "density")) for g in grids]
    total = sum(sizes)
    cap = sizes[0] + 70          # ends inside the second cloud, inside a wave's run of rows
    d = _dev(grids, hip_device)
    ws = torch.empty(_hip.voxel_cloud_ws_bytes(2, 1287) // 8, dtype=torch.int64, device=hip_device)
    offsets = torch.empty(3, dtype=torch.int64, device=hip_device)
    bad = torch.empty((2, 2), dtype=torch.int64, device=hip_device)
    rows = torch.full((total + 5, 6), -7.0, dtype=torch.float64, device=hip_device)
    xyz = torch.full((total + 5, 3), -7.0, dtype=torch.float64, device=hip_device)
    rgb = torch.full((total + 5, 3), 4242, dtype=torch.int16, device=hip_device)
    _hip.voxel_cloud_count(d, _hip.SN_CLOUD_DENSITY, 10, None, ws, offsets, bad)
    _hip.voxel_cloud_scatter(d, _hip.SN_CLOUD_DENSITY, 10, None, None, ws, offsets, rows, xyz, rgb, capacity=cap)
    assert offsets.cpu().tolist() == [0, sizes[0], total], "offsets hold the true sizes"
    assert _same(rows[:cap], want[:cap]) and bool((rows[cap:] == -7.0).all())
    assert _same(xyz[:cap], want[:cap, :3]) and bool((xyz[cap:] == -7.0).all())
    assert np.array_equal(rgb[:cap].cpu().numpy().view(np.uint16), vc.rgb16(want[:cap, 3:])) and bool((rgb[cap:] == 4242).all())
    cloud = sna.voxel_cloud(d, "density", capacity=cap)
    assert cloud.rows.shape == (cap, 6) and _same(cloud.rows, want[:cap]) and int(cloud.offsets[-1]) == total
    with pytest.raises(sna.HipLibraryError, match="capacity"):
        cloud.tile(1)


# ---- 4. NaN and colours outside [0, 255] -----------------------------------------------------------------------------------------
def test_density_nan_is_counted_and_the_mirror_raises(hip_device):
    grid = vc.seam_grid((9, 8, 7), 10, np.float64, seed=21)
    grid[2, 3, 4] = np.nan
    grid[8, 7, 6] = np.nan
    grid[0, 0, 0], grid[0, 0, 1] = 1.75, -np.inf
    want = vc.restate(grid, "density")
    nan, out = vc.bad_counts(grid, "density")
    assert nan == 2 and out >= 2
    cloud = sna.voxel_cloud(_dev(grid, hip_device)[None], "density")
    assert cloud.bad.cpu().tolist() == [[nan, out]]
    assert _same(cloud.rows, want)
    at = np.flatnonzero(np.isnan(want[:, 4]))
    got = cloud.rows.cpu().numpy()
    assert len(at) == 2 and np.all(got[at, 3] == 255.0) and np.isnan(got[at, 4:]).all(), "(255, NaN, NaN)"
    with pytest.raises(ValueError, match="NaN"):
        cloud.check()
    with pytest.raises(ValueError, match="NaN"):
        sna.plot_voxelgrid(grid, "density", plot=False)
    # ranges drops a NaN (NaN > lin[1] is false): nothing to count, nothing raised
    rows = sna.plot_voxelgrid(grid, "ranges", plot=False)
    assert _same(rows, vc.restate(grid, "ranges", 10, vc.jet_table(10)))


# ---- 5. desc: voxel centres, padding cells ---------------------------------------------------------------------------------------
def _tiles(seed, extents, n=4000):
    rng = np.random.default_rng(seed)
    return [rng.uniform(0.0, 1.0, (n, 3)) * e + 540000.0 for e in extents]


def test_desc_of_an_n_mode_batch(hip_device):
    tiles = _tiles(5, (30.0, 12.0))
    batch = sna.PointBatch.from_tiles(tiles, device=hip_device)
    g = sna.voxelize_batch(batch, (7, 6, 5), want_density=True, want_occ=True)       # grids [B,1,5,7,6]
    desc = g.desc.cpu().numpy()
    for grids, mode in ((g.density, "density"), (g.density, "ranges"), (g.occ, "density")):
        cloud = sna.voxel_cloud(grids, mode, desc=g.desc)
        for b in range(2):
            want = vc.restate_desc(grids[b, 0].cpu().numpy(), desc[b], mode, 10, _table(mode, 10))
            assert len(want) > 0 and _same(cloud.tile(b), want), (mode, b)
            assert want[:, 0].min() > 540000.0, "scan coordinates"


def test_desc_of_a_size_mode_batch_leaves_padding_cells_out(hip_device):
    tiles = _tiles(6, (10.0, 4.5))
    batch = sna.PointBatch.from_tiles(tiles, device=hip_device)
    g = sna.voxelize_batch(batch, (12, 12, 12), want_density=True, voxel_dims=(1.0, 1.0, 1.0))
    dims = g.dims.cpu().tolist()
    assert g.status.cpu().tolist() == [0, 0] and max(dims[1]) < 12, "the second tile is padded"
    desc = g.desc.cpu().numpy()
    grids = g.density.clone()
    keep = vc.desc_keep(desc[1], 12, 12, 12)
    assert 0 < keep.sum() < keep.size
    grids[1, 0][_dev(~keep, hip_device)] = 0.75          # what a convolution writes into the padding
    host = grids[:, 0].cpu().numpy()
    for mode in vc.MODES:
        cloud = sna.voxel_cloud(grids, mode, desc=g.desc)
        for b in range(2):
            want = vc.restate_desc(host[b], desc[b], mode, 10, _table(mode, 10))
            assert len(want) > 0 and np.isfinite(want).all()
            assert _same(cloud.tile(b), want), (mode, b)
        assert len(vc.restate(host[1], mode, 10, _table(mode, 10))) > cloud.sizes()[1], "without desc the padding shows"
        assert cloud.bad.cpu().tolist() == [list(vc.bad_counts(host[b], mode, vc.desc_keep(desc[b], 12, 12, 12)))
                                            for b in range(2)]


# ---- 6. rgb16 --------------------------------------------------------------------------------------------------------------------
def test_rgb16_against_the_restatement(hip_device):
    grid = vc.seam_grid((13, 11, 9), 10, np.float64, seed=31)
    grid[1, 1, 1], grid[1, 1, 2], grid[1, 1, 3] = np.nan, 1.75, 127.5 / 255.0
    for mode in vc.MODES:
        want = vc.restate(grid, mode, 10, _table(mode, 10))
        cloud = sna.voxel_cloud(_dev(grid, hip_device)[None], mode, las=True)
        assert cloud.rows is None and cloud.rgb.dtype == torch.uint16
        assert _same(cloud.xyz, want[:, :3])
        assert np.array_equal(cloud.rgb.cpu().view(torch.int16).numpy().view(np.uint16), vc.rgb16(want[:, 3:])), mode


# ---- 7. capture ------------------------------------------------------------------------------------------------------------------
def test_capture_and_replay_on_a_changed_grid(hip_device):
    shape = (2, 13, 11, 9)
    cases = [np.stack([vc.seam_grid(shape[1:], 10, np.float32, seed=s + b) for b in range(2)]) for s in (50, 60)]
    wants = [[vc.restate(g, "ranges", 10, vc.jet_table(10)) for g in c] for c in cases]
    capacity = max(sum(len(w) for w in ws) for ws in wants) + 9
    d = _dev(cases[0], hip_device)
    sna.voxel_cloud(d, "ranges", capacity=capacity)                 # (an eager call first: kernels are loaded)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cloud = sna.voxel_cloud(d, "ranges", capacity=capacity)
    for k in (0, 1, 0):
        d.copy_(torch.from_numpy(cases[k]))
        graph.replay()
        torch.cuda.synchronize()
        want = np.concatenate(wants[k])
        assert cloud.offsets.cpu().tolist() == [0, len(wants[k][0]), len(want)]
        assert _same(cloud.rows[:len(want)], want)
    assert len(np.concatenate(wants[0])) != len(np.concatenate(wants[1]))


# ---- 8. LAS ----------------------------------------------------------------------------------------------------------------------
def test_write_voxel_cloud_las_reads_back(hip_device, tmp_path):
    grids = np.stack([vc.seam_grid((9, 8, 7), 10, np.float64, seed=s) for s in (71, 72)])
    cloud = sna.voxel_cloud(_dev(grids, hip_device), "ranges", las=True)
    sizes = cloud.sizes()
    for k, n in ((1, sizes[1]), (None, sum(sizes))):
        path = str(tmp_path / f"cloud_{k}.las")
        written = sna.write_voxel_cloud_las(path, cloud, k=k, scale=(1.0, 1.0, 1.0), offset=(0.0, 0.0, 0.0))
        assert written.point_format == 2 and written.n_points == n and written.bad == (0, 0)
        scan = sna.read_las(path, device=hip_device)
        assert scan.xyz.shape == (n, 3)
        want = np.concatenate([vc.restate(g, "ranges", 10, vc.jet_table(10)) for g in (grids if k is None else grids[k:k + 1])])
        assert np.array_equal(scan.xyz.cpu().numpy(), want[:, :3]), "indices survive a unit grid"
        raw = np.fromfile(path, dtype=np.uint8)[written.data_offset:].reshape(n, written.record_length)
        rgb = np.ascontiguousarray(raw[:, 20:26]).view("<u2")
        assert np.array_equal(rgb, vc.rgb16(want[:, 3:]))
    with pytest.raises(sna.HipLibraryError, match="las=True"):
        sna.write_voxel_cloud_las(str(tmp_path / "x.las"), sna.voxel_cloud(_dev(grids, hip_device), "ranges"))
