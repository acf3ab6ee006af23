"""Scan merge on the device (K19: sn_scan_merge, scene_net_amd.scan_merge) against the numpy oracle of scan_merge_cases, the
product's own earlier path (sn_gather_points + merge_to_scan), a replayed graph, and the drivers on top (segment_scan,
classify_las).  MAX and INTERIOR are compared bit for bit (a NaN's payload aside), MEAN bit for bit against the oracle's
fp64 sum in region order, cover exactly."""
import os

import numpy as np
import pytest
import torch

import scene_net_amd as sna
from scene_net_amd import _hip
from scene_net_amd.scan_merge import _GridPipeline, group_batch, tile_groups

import crops_cases as cc
import scan_merge_cases as mc

pytestmark = pytest.mark.gpu

GUARD = 64
NP_DT = {torch.float32: np.float32, torch.float64: np.float64}


def _dev(a, dev, dtype=None):
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(dev)


def _run(dev, grid, desc, pts, regions, kinds, tile_of, rule, fill, want_cover=True):
    """(out [C, n], cover [n] | None) as numpy, after checking that nothing beyond out[:, :n] and cover[:n] was written"""
    C, n = grid.shape[1], pts.shape[0]
    tdt = torch.float32 if grid.dtype == np.float32 else torch.float64
    buf = torch.full((C * n + GUARD,), -123.0, dtype=tdt, device=dev)
    cbuf = torch.full((n + GUARD,), -77, dtype=torch.int32, device=dev)
    out, cover = buf[:C * n].view(C, n), cbuf[:n]
    _hip.scan_merge(_dev(grid, dev), _dev(desc, dev), _dev(pts, dev), _dev(regions, dev), _dev(kinds, dev, torch.int32),
                    _dev(tile_of, dev, torch.int32), rule, fill, out, cover if want_cover else None)
    assert bool((buf[C * n:] == -123.0).all()) and bool((cbuf[n:] == -77).all()), "wrote beyond its outputs"
    if not want_cover:
        assert bool((cbuf == -77).all())
    return out.cpu().numpy(), (cover.cpu().numpy() if want_cover else None)


def _check(dev, grid, desc, dims, pts, regions, kinds, tile_of, fill=-3.5, own=None, rules=mc.RULES, what=""):
    for rule in rules:
        want, want_cover = mc.merge_oracle(grid, desc, dims, pts, regions, kinds, tile_of, rule, fill, own)
        got, cover = _run(dev, grid, desc, pts, regions, kinds, tile_of, rule, fill)
        assert np.array_equal(cover, want_cover), f"{what} rule {rule}: cover"
        assert mc.same_bits(got, want), f"{what} rule {rule}: {int((got != want).sum())} values differ"


# ---- 1. the cases against the oracle ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("dims", mc.DIMS)
def test_main_case(hip_device, dims, channels, dtype):
    pts, regions, kinds, ties = mc.main_scan()
    desc, _ = mc.main_desc(dims)
    grid = mc.random_grid(10, channels, dims, dtype, 11)
    _check(hip_device, grid, desc, dims, pts, regions, kinds, None, what="main")
    # the tie points: the lowest region index wins
    got, cover = _run(hip_device, grid, desc, pts, regions, kinds, None, mc.INTERIOR, 0.0)
    import binning_cases as bc
    for i in ties:
        f = bc.expected_flat(desc[mc.TIE_WINNER], dims, pts[i:i + 1])[0]
        assert np.array_equal(got[:, i], grid.reshape(10, channels, -1)[mc.TIE_WINNER, :, f])
    assert cover[ties].tolist() == [2, 2, 4]
    # without cover the values are the same and cover's buffer is left alone
    alone, _ = _run(hip_device, grid, desc, pts, regions, kinds, None, mc.INTERIOR, 0.0, want_cover=False)
    assert mc.same_bits(alone, got)


@pytest.mark.parametrize("n", mc.SEAM_N)
def test_seam_sizes_n(hip_device, n):
    pts, regions, kinds, _ = mc.main_scan()
    dims = mc.DIMS[0]
    desc, _ = mc.main_desc(dims)
    _check(hip_device, mc.random_grid(10, 1, dims, np.float32, 12), desc, dims, pts[:n], regions, kinds, None, what=f"n={n}")


@pytest.mark.parametrize("K", mc.SEAM_K)
def test_seam_sizes_k(hip_device, K):
    pts, regions, kinds, _ = mc.main_scan()
    dims = mc.DIMS[0]
    desc, _ = mc.main_desc(dims)
    idx = mc.repeated_regions(K)            # regions share tiles: tile_of[k] = the main region row k repeats
    _check(hip_device, mc.random_grid(10, 3, dims, np.float64, 13), desc, dims, pts, regions[idx], kinds[idx], idx,
           what=f"K={K}")


def test_tile_of_variants(hip_device):
    pts, regions, kinds, _ = mc.main_scan()
    dims = mc.DIMS[1]
    desc, _ = mc.main_desc(dims)
    grid = mc.random_grid(10, 1, dims, np.float32, 14)
    holes = np.arange(10, dtype=np.int32)
    holes[[1, 4]] = -1
    holes[7], holes[9] = 10, 1 << 30                    # outside 0..B-1: no tile
    _check(hip_device, grid, desc, dims, pts, regions, kinds, holes, what="holes")
    perm = np.random.default_rng(3).permutation(10).astype(np.int32)
    g2, d2 = np.empty_like(grid), np.empty_like(desc)
    g2[perm], d2[perm] = grid, desc                     # tile perm[k] holds region k's grid
    _check(hip_device, g2, d2, dims, pts, regions, kinds, perm, what="permutation")
    want, _ = mc.merge_oracle(grid, desc, dims, pts, regions, kinds, None, mc.MEAN, 0.0)
    got, _ = _run(hip_device, g2, d2, pts, regions, kinds, perm, mc.MEAN, 0.0)
    assert mc.same_bits(got, want)
    shared = np.array([0, 0, 2, 3, 3, 5, 6, 7, 8, 9], dtype=np.int32)      # regions 1 and 4 read a neighbour's tile
    _check(hip_device, grid, desc, dims, pts, regions, kinds, shared, what="shared")
    _check(hip_device, grid, desc, dims, pts, regions[:, [0, 1, 2, 3]], None, None, what="kinds null: all discs")
    # fewer tiles than regions
    _check(hip_device, grid[:4], desc[:4], dims, pts, regions, kinds, np.array([0, 1, 2, 3, -1, -1, 3, 2, 1, 0], dtype=np.int32),
           what="B < K")


@pytest.mark.parametrize("kind", ["foreign", "sized"])
def test_foreign_descriptors(hip_device, kind):
    pts, regions, kinds, _ = mc.main_scan()
    dims = mc.CAPACITY if kind == "sized" else mc.DIMS[0]
    desc, own = mc.main_desc(dims, kind)
    for dtype in (np.float32, np.float64):
        _check(hip_device, mc.random_grid(10, 2, dims, dtype, 15), desc, dims, pts, regions, kinds, None, own=own, what=kind)


def test_long_edge_table(hip_device):
    """7203 edges: table and the chunk's z no longer fit 64 KiB of LDS together, so a member loads its z from memory"""
    pts, regions, kinds, _ = mc.main_scan()
    dims = (7200, 1, 1)
    desc, _ = mc.main_desc(dims)
    _check(hip_device, mc.random_grid(10, 1, dims, np.float32, 20), desc, dims, pts, regions, kinds, None, what="long table")


def test_nan_predictions(hip_device):
    pts, regions, kinds, _ = mc.main_scan()
    dims = mc.DIMS[0]
    desc, _ = mc.main_desc(dims)
    grid = mc.random_grid(10, 1, dims, np.float32, 16, nans=30)      # a quarter of every tile's cells
    want, cover = mc.merge_oracle(grid, desc, dims, pts, regions, kinds, None, mc.MAX, 0.0)
    assert int(np.isnan(want[0, cover >= 2]).sum()) > 100 and int((~np.isnan(want[0, cover >= 2])).sum()) > 100
    _check(hip_device, grid, desc, dims, pts, regions, kinds, None, fill=float("nan"), what="NaN")


def test_odd_regions_and_points(hip_device):
    """K9's non-finite points and degenerate regions, every region reading one tile: membership is K9's, literally"""
    pts, _, regions, kinds = cc.nonfinite_case()
    dims = mc.DIMS[0]
    finite = pts[np.isfinite(pts).all(axis=1)]
    row, _ = mc.desc_row(finite, dims)
    K = regions.shape[0]
    _check(hip_device, mc.random_grid(1, 1, dims, np.float64, 17), row[None], dims, pts, regions, kinds,
           np.zeros(K, dtype=np.int32), what="odd")


# ---- 2. against the product's earlier path ------------------------------------------------------------------------------
def test_equals_gather_and_merge_to_scan(hip_device):
    pts, regions, kinds, _ = mc.main_scan()
    pts = pts[np.isfinite(pts).all(axis=1)]
    n = pts.shape[0]
    d_pts, d_reg, d_kin = _dev(pts, hip_device), _dev(regions, hip_device), _dev(kinds, hip_device, torch.int32)
    # an eleventh region that holds nothing: point_batch drops it, kept says so
    d_reg = torch.cat([d_reg, torch.tensor([[0.0, 0.0, 1.0, 1.0]], dtype=torch.float64, device=hip_device)])
    d_kin = torch.cat([d_kin, torch.ones(1, dtype=torch.int32, device=hip_device)])
    crops = sna.crop_regions(d_pts, d_reg, d_kin)
    batch, kept = crops.point_batch()
    assert kept == list(range(10))
    for dims in ((8, 8, 8), (5, 7, 3)):
        grids = sna.voxelize_batch(batch, dims)
        pred = torch.randn((10, 2, dims[2], dims[0], dims[1]), device=hip_device)
        pp = sna.point_predictions(pred, batch, grids, fill=-9.0)
        got, cover = sna.scan_predictions(pred, d_pts, d_reg, d_kin, grids, kept, rule="max", fill=-9.0, want_cover=True)
        for c in range(2):
            assert torch.equal(got[c], sna.merge_to_scan(pp[c], crops.src_rows(), n, fill=-9.0))
        seen = torch.zeros(n, dtype=torch.int32, device=hip_device)
        seen.index_add_(0, crops.src_rows(), torch.ones_like(crops.src_rows(), dtype=torch.int32))
        assert torch.equal(cover, seen)


# ---- 3. capture -------------------------------------------------------------------------------------------------------------
def test_replay_follows_the_device_tables(hip_device):
    pts, regions, kinds, _ = mc.main_scan()
    dims = mc.DIMS[1]
    desc, _ = mc.main_desc(dims)
    n = pts.shape[0]
    d_pts, d_desc = _dev(pts, hip_device), _dev(desc, hip_device)
    d_reg, d_kin = _dev(regions, hip_device), _dev(kinds, hip_device, torch.int32)
    d_tile = torch.arange(10, dtype=torch.int32, device=hip_device)
    d_grid = _dev(mc.random_grid(10, 1, dims, np.float32, 18), hip_device)
    out = torch.empty((1, n), dtype=torch.float32, device=hip_device)
    cover = torch.empty((n,), dtype=torch.int32, device=hip_device)
    side = torch.cuda.Stream(device=hip_device)
    side.wait_stream(torch.cuda.current_stream(hip_device))
    with torch.cuda.stream(side):
        _hip.scan_merge(d_grid, d_desc, d_pts, d_reg, d_kin, d_tile, mc.INTERIOR, 2.0, out, cover)      # (loads the kernel)
    torch.cuda.current_stream(hip_device).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _hip.scan_merge(d_grid, d_desc, d_pts, d_reg, d_kin, d_tile, mc.INTERIOR, 2.0, out, cover)
    # new contents, in place: other values, the boxes moved by 1.25 m, two regions without a tile and two swapped
    d_grid.copy_(_dev(mc.random_grid(10, 1, dims, np.float32, 19), hip_device))
    d_reg[:9] += torch.tensor([1.25, -1.25, 1.25, -1.25], dtype=torch.float64, device=hip_device)
    d_tile.copy_(torch.tensor([0, 1, -1, 3, 5, 4, 6, -1, 8, 9], dtype=torch.int32, device=hip_device))
    out.fill_(-1.0)
    cover.fill_(-1)
    graph.replay()
    torch.cuda.synchronize()
    fresh = torch.empty_like(out)
    fresh_cover = torch.empty_like(cover)
    _hip.scan_merge(d_grid, d_desc, d_pts, d_reg, d_kin, d_tile, mc.INTERIOR, 2.0, fresh, fresh_cover)
    assert mc.same_bits(out.cpu().numpy(), fresh.cpu().numpy()) and torch.equal(cover, fresh_cover)
    want, want_cover = mc.merge_oracle(d_grid.cpu().numpy(), desc, dims, pts, d_reg.cpu().numpy(), kinds, d_tile.cpu().numpy(),
                                       mc.INTERIOR, 2.0)
    assert mc.same_bits(out.cpu().numpy(), want) and np.array_equal(cover.cpu().numpy(), want_cover)


# ---- 4. segment_scan --------------------------------------------------------------------------------------------------------
def _three_tile_scan(golden_dir):
    """the scan test_gpu_crops.test_whole_scan_inference_loop builds: three shifted copies of the golden tile, interleaved,
    and one point in no box"""
    a = np.load(os.path.join(golden_dir, "ts40k_sample575_subset.npy"))
    m = a.shape[0] // 3
    tiles = []
    for j in range(3):
        t = np.ascontiguousarray(a[j * m:(j + 1) * m, :3])
        t[:, 0] += 1000.0 * j
        tiles.append(t)
    n = 3 * m + 1
    scan = np.empty((n, 3))
    for j in range(3):
        scan[j:3 * m:3] = tiles[j]
    scan[-1] = [tiles[0][:, 0].min() - 5000.0, tiles[0][0, 1], tiles[0][0, 2]]
    boxes = np.array([[t[:, 0].min(), t[:, 1].min(), t[:, 0].max(), t[:, 1].max()] for t in tiles])
    return scan, boxes, m


def test_segment_scan(hip_device, golden_dir):
    scan, boxes, m = _three_tile_scan(golden_dir)
    n = scan.shape[0]
    d_scan, d_box = _dev(scan, hip_device), _dev(boxes, hip_device)
    d_kin = torch.ones(3, dtype=torch.int32, device=hip_device)
    torch.manual_seed(0)
    model = sna.SceneNet({"cy": 2, "cone": 1, "neg": 1}, (9, 9, 9)).to(hip_device)
    # the earlier recipe, as test_whole_scan_inference_loop runs it
    crops = sna.crop_regions(d_scan, d_box, d_kin)
    batch, kept = crops.point_batch()
    with torch.no_grad():
        _, pp = sna.ScenePipeline(model, (32, 32, 32), per_point=True)(batch)
    merged = sna.merge_to_scan(pp[0], crops.src_rows(), n, fill=-1.0)
    seg = sna.segment_scan(model, d_scan, d_box, d_kin, grid=(32, 32, 32), rule="max", batch_tiles=3, fill=-1.0)
    assert isinstance(seg, sna.ScanSegmentation) and seg.kept == [0, 1, 2] and seg.prob.shape == (1, n)
    assert torch.equal(seg.prob[0], merged)
    assert float(seg.prob[0, -1]) == -1.0 and int(seg.cover[-1]) == 0 and bool((seg.cover[:-1] == 1).all())
    # two groups: the same pipeline by hand over the same groups, then one scan_predictions
    seg2 = sna.segment_scan(model, d_scan, d_box, d_kin, grid=(32, 32, 32), rule="interior", batch_tiles=2, fill=-1.0)
    groups = tile_groups(3, 2)
    assert [list(g) for g in groups] == [[0, 1], [2]]
    starts = np.concatenate([[0], np.cumsum(batch.sizes)])
    pipe = _GridPipeline(model, (32, 32, 32))
    preds, descs = [], []
    with torch.no_grad():
        for g in groups:
            out, grids = pipe(group_batch(batch, g, starts))
            preds.append(out.clone())
            descs.append(grids.desc.clone())
    by_hand, cover = sna.scan_predictions(torch.cat(preds), d_scan, d_box, d_kin, torch.cat(descs), kept, rule="interior",
                                          fill=-1.0, want_cover=True)
    assert torch.equal(seg2.prob, by_hand) and torch.equal(seg2.cover, cover)
    assert float(seg2.prob[0, -1]) == -1.0 and int(seg2.cover[-1]) == 0
    # regions None: the lattice over the scan's own xy box, made on the device
    seg3 = sna.segment_scan(model, d_scan[:3 * m:3], tile=12.0, overlap=2.0, grid=(32, 32, 32))
    assert seg3.regions.shape == (4, 4) and seg3.kept == [0, 1, 2, 3] and int(seg3.cover.max()) > 1
    assert seg3.regions.is_cuda and seg3.prob.shape == (1, m) and int(seg3.cover.min()) >= 1 and int(seg3.cover.max()) <= 4
    assert bool(torch.isfinite(seg3.prob).all())


# ---- 5. classify_las --------------------------------------------------------------------------------------------------------
def test_classify_las(hip_device, golden_dir, tmp_path):
    scan, _, m = _three_tile_scan(golden_dir)
    xyz = _dev(scan[:3 * m:3], hip_device)
    n = xyz.shape[0]
    rng = np.random.default_rng(5)
    original = _dev(rng.integers(0, 10, n).astype(np.float64), hip_device)
    gps = _dev(rng.random(n) * 1e5, hip_device)
    src, dst = str(tmp_path / "in.las"), str(tmp_path / "out.las")
    sna.write_las(src, xyz, original, gps_time=gps, point_format=1)
    torch.manual_seed(0)
    model = sna.SceneNet({"cy": 2, "cone": 1, "neg": 1}, (9, 9, 9)).to(hip_device)
    back = sna.read_las(src, device=hip_device)
    probe = sna.segment_scan(model, back.xyz, tile=12.0, overlap=2.0, grid=(32, 32, 32))
    tau = 0.5 * (float(probe.prob[0].min()) + float(probe.prob[0].max()))      # some points change class, some do not
    seg = sna.classify_las(src, dst, model, tau, tile=12.0, overlap=2.0, grid=(32, 32, 32))
    assert torch.equal(seg.prob, probe.prob)
    want = torch.where(seg.prob[0] >= tau, torch.full_like(original, 15.0), back.classes)
    assert 0 < int((want == 15.0).sum()) < n
    out = sna.read_las(dst, device=hip_device)
    assert torch.equal(out.classes, want) and torch.equal(out.xyz, back.xyz)
    # every other byte of the file is src's
    a, b = np.fromfile(src, dtype=np.uint8), np.fromfile(dst, dtype=np.uint8)
    h = sna.read_las_header(src)
    assert a.shape == b.shape and h.point_format == 1
    ra = a[h.data_offset:h.data_offset + h.payload_bytes].reshape(n, h.record_length).copy()
    rb = b[h.data_offset:h.data_offset + h.payload_bytes].reshape(n, h.record_length).copy()
    assert np.array_equal(ra[:, 15] & 0xE0, rb[:, 15] & 0xE0)
    ra[:, 15] = rb[:, 15] = 0
    assert np.array_equal(ra, rb)
    assert np.array_equal(a[:h.data_offset], b[:h.data_offset]) and np.array_equal(a[h.data_offset + h.payload_bytes:],
                                                                                   b[h.data_offset + h.payload_bytes:])
