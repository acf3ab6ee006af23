"""Scan crops on the device (K9: sn_crop_count / sn_crop_scatter, scene_net_amd.crops) against the numpy oracle of
crops_cases -- `scan[mask]` in the reference's own expressions.  Every comparison is exact: integers as they are, fp64 as
int64 views."""
import os

import numpy as np
import pytest
import torch

import scene_net_amd as sna
from scene_net_amd import _hip

import crops_cases as cc
from scene_net_amd.crops import lattice_boxes

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A5A5A5A5A
GUARD = 64


def _dev(a, dev, dtype, offset_by_one=False):
    """`a` on the device: 16-byte aligned (torch's allocations are), or offset by one element from such an address"""
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dtype)
    if not offset_by_one:
        out = t.to(dev)
        assert out.data_ptr() % 16 == 0
        return out
    buf = torch.empty(t.numel() + 1, dtype=dtype, device=dev)
    view = buf[1:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == t.element_size() % 16 and view.is_contiguous()
    return view


def _crop(dev, pts, labels, regions, kinds, want_src=True, offset_by_one=False):
    return sna.crop_regions(_dev(pts, dev, torch.float64, offset_by_one), _dev(regions, dev, torch.float64, offset_by_one),
                            _dev(kinds, dev, torch.int32, offset_by_one), _dev(labels, dev, torch.float64, offset_by_one),
                            want_src=want_src)


def _bits(t):
    return t.cpu().contiguous().view(torch.int64).numpy()


def _assert_equals_oracle(crops, pts, labels, regions, kinds, what=""):
    offsets, rows, lab, src = cc.crop_oracle(pts, labels, regions, kinds)
    assert np.array_equal(crops.offsets.cpu().numpy(), offsets), f"{what}: offsets"
    assert crops.pts.shape == (offsets[-1], 3)
    assert np.array_equal(_bits(crops.pts), cc.bits(rows)), f"{what}: rows"
    if labels is None:
        assert crops.labels is None
    else:
        assert np.array_equal(_bits(crops.labels), cc.bits(lab)), f"{what}: labels"
    if crops.src is not None:
        assert np.array_equal(crops.src.cpu().numpy(), src), f"{what}: src"
    return offsets, src


# ---- 1. seams ----------------------------------------------------------------------------------------------------------
def _seam_sizes():
    c = _hip.crops_chunk_points()
    return [1, 63, 64, 65, 255, 257, c - 1, c, c + 1, 3 * c + 17]


SEAM_K = (1, 2, 31, 33, 64, 65, 300)
# (labels, src, buffers offset by one element)
SEAM_VARIANTS = ((True, True, False), (False, False, True), (True, False, True), (False, True, False))


@pytest.mark.parametrize("which", range(10))
def test_seams_of_chunks_and_region_tiles(hip_device, which):
    n = _seam_sizes()[which]
    pts, labels, regions, kinds = cc.random_case(n, max(SEAM_K), seed=100 + which)
    members = 0
    for j, K in enumerate(SEAM_K):
        for with_labels, with_src, off1 in SEAM_VARIANTS[2 * ((which + j) % 2):][:2]:
            crops = _crop(hip_device, pts, labels if with_labels else None, regions[:K], kinds[:K], with_src, off1)
            assert (crops.src is not None) is with_src
            offsets, _ = _assert_equals_oracle(crops, pts, labels if with_labels else None, regions[:K], kinds[:K],
                                               f"n={n} K={K} labels={with_labels} src={with_src} offset={off1}")
            members += int(offsets[-1])
    assert members > 0 or n < 64


def test_prefix_carries_into_the_second_scan_tile(hip_device):
    """The prefix kernel scans a region's row in tiles of 256 threads x 8 slots = 2048 chunks and carries the running total
    from one tile to the next: one chunk more than a tile, so the prefixes of chunk 2048 and the totals hold a carry.  (Not
    a case of the seam test above: its K = 300 regions would cost the oracle minutes at this size.)"""
    c = _hip.crops_chunk_points()
    tile = 256 * 8                                   # kScanThreads * kScanItems of scan.h
    n = (tile + 1) * c + 17
    rng = np.random.default_rng(2049)
    pts = cc.ORIGIN + rng.random((n, 3)) * np.array([60.0, 60.0, 40.0])
    labels = rng.choice(np.array([0.0, 2.0, 15.0, 16.0]), n)
    x0, y0 = cc.ORIGIN[:2]
    regions = np.array([[x0 - 1.0, y0 - 1.0, x0 + 30.0, y0 + 61.0],            # a box: the left half of the scan
                        [x0 + 40.0, y0 + 20.0, 12.5, 0.0]])                      # a disc
    kinds = np.array([cc.BOX, cc.DISC], dtype=np.int32)
    crops = _crop(hip_device, pts, labels, regions, kinds)
    offsets, src = _assert_equals_oracle(crops, pts, labels, regions, kinds, "carry")
    assert 0.45 * n < offsets[1] < 0.55 * n
    for k in range(2):                               # members on both sides of the seam: a dropped carry cannot pass
        s = src[offsets[k]:offsets[k + 1]]
        assert (s < tile * c).sum() > 1000 and (s >= tile * c).sum() > 10, f"region {k}"


def test_all_discs_when_kinds_is_null(hip_device):
    pts, labels, regions, _ = cc.random_case(2500, 40, seed=7, mixed=False)
    crops = _crop(hip_device, pts, labels, regions, None)
    assert crops.kinds is None
    offsets, _ = _assert_equals_oracle(crops, pts, labels, regions, None, "null kinds")
    assert offsets[-1] > 2500, "overlapping discs repeat rows"


# ---- 2. boundary, contraction, non-finite ----------------------------------------------------------------------------------
def test_exact_boundaries(hip_device):
    pts, labels, regions, kinds, claims = cc.boundary_case()
    crops = _crop(hip_device, pts, labels, regions, kinds)
    offsets, src = _assert_equals_oracle(crops, pts, labels, regions, kinds, "boundary")
    got_src = crops.src.cpu().numpy()
    for k, i, member in claims:
        assert (i in got_src[offsets[k]:offsets[k + 1]]) is member, (k, i, member)


def test_chunk_reject_keeps_a_point_on_the_rim_of_its_chunk(hip_device):
    """every workgroup's xy box touches its regions in one point only: the conservative skip must keep the chunk at r and
    may drop it at nextafter(r, 0)"""
    pts, labels, regions, kinds, claims = cc.rim_case(_hip.crops_chunk_points())
    crops = _crop(hip_device, pts, labels, regions, kinds)
    offsets, _ = _assert_equals_oracle(crops, pts, labels, regions, kinds, "rim")
    got_src = crops.src.cpu().numpy()
    for k, i, member in claims:
        assert (i in got_src[offsets[k]:offsets[k + 1]]) is member, (k, i, member)


def test_contraction_set(hip_device):
    pts, labels, regions, kinds, count = cc.contraction_case()
    assert count >= 64
    crops = _crop(hip_device, pts, labels, regions, kinds)
    _assert_equals_oracle(crops, pts, labels, regions, kinds, "contraction")
    # each draw against its own disc, where a contracted sum would decide the other way
    own = np.array([bool(cc.disc_mask(pts[i:i + 1], regions[i, :2], float(regions[i, 2]))[0]) for i in range(count)])
    off, src = crops.offsets.cpu().numpy(), crops.src.cpu().numpy()
    got = np.array([i in src[off[i]:off[i + 1]] for i in range(count)])
    assert np.array_equal(got, own) and own.any() and not own.all()


def test_nonfinite_and_odd_values_keep_their_bits(hip_device):
    pts, labels, regions, kinds = cc.nonfinite_case()
    crops = _crop(hip_device, pts, labels, regions, kinds)
    offsets, src = _assert_equals_oracle(crops, pts, labels, regions, kinds, "non-finite")
    # the box of infinite bounds holds every point without a NaN in x or y, whatever z and the label carry
    k = 9
    want = np.flatnonzero(~np.isnan(pts[:, 0]) & ~np.isnan(pts[:, 1]))
    assert np.array_equal(src[offsets[k]:offsets[k + 1]], want)
    carried = set(_bits(crops.pts[offsets[k]:offsets[k + 1]]).reshape(-1).tolist()) | \
        set(_bits(crops.labels[offsets[k]:offsets[k + 1]]).tolist())
    for pattern in (0x7ff8000000001234, 0xfff800000000beef, 0x7ff0000000000077, 0x8000000000000000, 1):
        assert np.array(pattern, dtype=np.uint64).view(np.int64).item() in carried, hex(pattern)


# ---- 3. stability and overlap ----------------------------------------------------------------------------------------------
def test_repeated_nested_and_covering_regions(hip_device):
    pts, labels, _, _ = cc.random_case(3000, 1, seed=21)
    c = cc.ORIGIN[:2] + 30.0
    regions = np.array([[c[0], c[1], 12.0, 0.0], [c[0], c[1], 12.0, 0.0], [c[0], c[1], 5.0, 0.0], [c[0], c[1], 40.0, 0.0],
                        [-np.inf, -np.inf, np.inf, np.inf]])
    kinds = np.array([0, 0, 0, 0, 1], dtype=np.int32)
    crops = _crop(hip_device, pts, labels, regions, kinds)
    off, _ = _assert_equals_oracle(crops, pts, labels, regions, kinds, "overlap")
    t = [crops.tile(k) for k in range(5)]
    assert torch.equal(t[0][0], t[1][0]) and torch.equal(t[0][2], t[1][2]) and 0 < t[0][0].shape[0] < 3000
    s_small, s_mid, s_big = (set(t[k][2].cpu().tolist()) for k in (2, 0, 3))
    assert s_small < s_mid < s_big
    for k in range(5):
        assert torch.all(t[k][2][1:] > t[k][2][:-1]), "scan order"
    assert torch.equal(t[4][2], torch.arange(3000, device=hip_device))
    assert np.array_equal(_bits(t[4][0]), cc.bits(pts)) and np.array_equal(_bits(t[4][1]), cc.bits(labels))


def _raw_call(dev, pts, labels, regions, kinds, capacity, rows):
    """the two entries back to back on sentinel-filled buffers of rows + GUARD rows; returns (offsets, pts, labels, src)
    as int64 host arrays"""
    d_pts, d_lab = _dev(pts, dev, torch.float64), _dev(labels, dev, torch.float64)
    d_reg, d_kinds = _dev(regions, dev, torch.float64), _dev(kinds, dev, torch.int32)
    n, K = pts.shape[0], regions.shape[0]
    ws = torch.empty(_hip.crops_ws_bytes(n, K) // 8, dtype=torch.int64, device=dev)
    offsets = torch.full((K + 1,), SENTINEL, dtype=torch.int64, device=dev)
    total = rows + GUARD
    out_pts = torch.full((total, 3), SENTINEL, dtype=torch.int64, device=dev).view(torch.float64)
    out_lab = torch.full((total,), SENTINEL, dtype=torch.int64, device=dev).view(torch.float64)
    out_src = torch.full((total,), SENTINEL, dtype=torch.int64, device=dev)
    _hip.crop_count(d_pts, d_reg, d_kinds, ws, offsets)
    _hip.crop_scatter(d_pts, d_lab, d_reg, d_kinds, ws, offsets, out_pts, out_lab, out_src, capacity=capacity)
    torch.cuda.synchronize()
    return offsets.cpu().numpy(), _bits(out_pts), _bits(out_lab), out_src.cpu().numpy()


def test_all_regions_empty_touch_nothing(hip_device):
    pts, labels, _, _ = cc.random_case(2100, 1, seed=22)
    regions = np.array([[0.0, 0.0, 10.0, 0.0], [1.0, 1.0, 0.0, 0.0], [cc.ORIGIN[0], cc.ORIGIN[1], np.nan, 0.0],
                        [cc.ORIGIN[0], cc.ORIGIN[1], np.inf, 0.0]])
    kinds = np.array([0, 1, 0, 5], dtype=np.int32)
    offsets, o_pts, o_lab, o_src = _raw_call(hip_device, pts, labels, regions, kinds, capacity=64, rows=64)
    assert np.array_equal(offsets, np.zeros(5, dtype=np.int64))
    assert np.all(o_pts == SENTINEL) and np.all(o_lab == SENTINEL) and np.all(o_src == SENTINEL)


# ---- 4. capacity -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ("total-1", "half", "zero", "exact"))
def test_capacity_bounds_the_writes_and_offsets_stay_true(hip_device, which):
    pts, labels, regions, kinds = cc.random_case(2600, 9, seed=23)
    offsets, rows, lab, src = cc.crop_oracle(pts, labels, regions, kinds)
    total = int(offsets[-1])
    assert total > 2600
    capacity = {"total-1": total - 1, "half": total // 2, "zero": 0, "exact": total}[which]
    got_off, o_pts, o_lab, o_src = _raw_call(hip_device, pts, labels, regions, kinds, capacity=capacity, rows=total)
    assert np.array_equal(got_off, offsets), "offsets hold the true sizes whatever the capacity"
    assert np.array_equal(o_pts[:capacity], cc.bits(rows)[:capacity])
    assert np.array_equal(o_lab[:capacity], cc.bits(lab)[:capacity])
    assert np.array_equal(o_src[:capacity], src[:capacity])
    assert np.all(o_pts[capacity:] == SENTINEL) and np.all(o_lab[capacity:] == SENTINEL) and np.all(o_src[capacity:] == SENTINEL)
    assert o_src.shape[0] == total + GUARD


def test_crop_regions_with_a_capacity_does_not_read_back(hip_device):
    pts, labels, regions, kinds = cc.random_case(1500, 4, seed=24)
    offsets, rows, lab, src = cc.crop_oracle(pts, labels, regions, kinds)
    total = int(offsets[-1])
    crops = sna.crop_regions(_dev(pts, hip_device, torch.float64), _dev(regions, hip_device, torch.float64),
                             _dev(kinds, hip_device, torch.int32), _dev(labels, hip_device, torch.float64), capacity=total + 100)
    assert crops.pts.shape == (total + 100, 3) and crops.src.shape == (total + 100,)
    assert np.array_equal(crops.offsets.cpu().numpy(), offsets)
    assert np.array_equal(_bits(crops.pts[:total]), cc.bits(rows)) and np.array_equal(crops.src[:total].cpu().numpy(), src)
    batch, kept = crops.point_batch()
    assert batch.total_points == total and batch.pts.shape[0] == total and kept == [k for k in range(4) if offsets[k + 1] > offsets[k]]


# ---- 5. golden tile ----------------------------------------------------------------------------------------------------------
def test_golden_tile_membership_and_mirrors(hip_device, golden_dir):
    tile = np.load(os.path.join(golden_dir, "ts40k_sample575_full.npz"))["tile"]
    g = np.load(os.path.join(golden_dir, "scan_crops.npz"))
    xyz, classes = np.ascontiguousarray(tile[:, :3]), np.ascontiguousarray(tile[:, 3])
    n = len(xyz)
    stored = cc.golden_crops(g)
    regions = np.stack([row for _, row, _ in stored])
    kinds = np.array([kind for _, _, kind in stored], dtype=np.int32)
    crops = _crop(hip_device, xyz, classes, regions, kinds)
    off, src = crops.offsets.cpu().numpy(), crops.src.cpu().numpy()
    want_sizes = {}
    for k, (name, _, _) in enumerate(stored):
        mask = np.zeros(n, dtype=bool)
        mask[src[off[k]:off[k + 1]]] = True
        assert np.array_equal(np.packbits(mask), g[name + "_bits"]), name
        want_sizes[name] = int(mask.sum())
    # the mirrors: the reference's row counts, shapes and dtypes
    d_xyz, d_cls = torch.from_numpy(xyz).to(hip_device), torch.from_numpy(classes).to(hip_device)
    centres = torch.from_numpy(g["at_centres"]).to(hip_device)
    for j, r in enumerate(g["at_radii"]):
        samples = sna.crop_at_locations(d_xyz, centres, radius=float(r), classes=d_cls)
        assert [tuple(s.shape) for s in samples] == [(want_sizes[f"at_{j}_{i}"], 4) for i in range(6)]
        assert all(s.dtype == torch.float64 and s.is_cuda for s in samples)
    assert [tuple(s.shape) for s in sna.crop_at_locations(d_xyz, centres, radius=3.0)] == \
        [(want_sizes[f"at_1_{i}"], 3) for i in range(6)]
    tower = d_xyz[d_cls == 15]
    for j, r in enumerate(g["tower_radii"]):
        rad, c = sna.crop_tower_radius(d_xyz, d_cls, tower, radius=float(r))
        assert tuple(rad.shape) == (want_sizes[f"tower_{j}"], 3) and rad.dtype == torch.float64
        assert tuple(c.shape) == (want_sizes[f"tower_{j}"],) and c.dtype == torch.int64
    half = int(g["two_split"][0])
    a, c = sna.crop_two_towers(d_xyz, d_cls, tower[:half], tower[half:])
    assert tuple(a.shape) == (want_sizes["two"], 3) and c.dtype == torch.int64 and tuple(c.shape) == (want_sizes["two"],)
    mask = np.unpackbits(g["two_bits"])[:n].astype(bool)
    assert np.array_equal(_bits(a), cc.bits(xyz[mask])) and np.array_equal(c.cpu().numpy(), classes[mask].astype(np.int64))
    samples = sna.crop_tower_samples(d_xyz, d_cls, [tower], radius=15)
    assert len(samples) == 1 and tuple(samples[0].shape) == (want_sizes["tower_2"], 4)


# ---- 6. mirrors and the tower mean ---------------------------------------------------------------------------------------------
def test_tower_radius_on_a_grid_where_every_mean_is_the_same(hip_device):
    """256 tower points on a 2^-10 grid: every partial sum is exact, so torch.mean and numpy's mean give the same centre"""
    rng = np.random.default_rng(31)
    pts, labels, _, _ = cc.random_case(4000, 1, seed=32)
    tower = np.column_stack([cc.ORIGIN[0] + 30 + rng.integers(-2048, 2048, 256) / 1024.0,
                             cc.ORIGIN[1] + 30 + rng.integers(-2048, 2048, 256) / 1024.0,
                             cc.ORIGIN[2] + rng.integers(0, 20 * 1024, 256) / 1024.0])
    centre = np.mean(tower, axis=0)
    assert np.array_equal(centre, np.array([float(sum(map(float, tower[:, a]))) / 256 for a in range(3)]))
    d_pts, d_lab = torch.from_numpy(pts).to(hip_device), torch.from_numpy(labels).to(hip_device)
    d_tower = torch.from_numpy(tower).to(hip_device)
    for radius in (0, 15):
        r = np.max(tower[:, 2]) - np.min(tower[:, 2]) if radius == 0 else radius
        mask = cc.disc_mask(pts, centre[:2], float(r))
        rad, c = sna.crop_tower_radius(d_pts, d_lab, d_tower, radius=radius)
        assert 0 < mask.sum() < 4000
        assert np.array_equal(_bits(rad), cc.bits(pts[mask])) and np.array_equal(c.cpu().numpy(), labels[mask].astype(np.int64))
    samples = sna.crop_tower_samples(d_pts, d_lab, [d_tower, d_tower[:128]], radius=15)
    assert len(samples) == 2 and np.array_equal(_bits(samples[0][:, :3]), cc.bits(pts[cc.disc_mask(pts, centre[:2], 15.0)]))
    want = np.column_stack([pts, labels])[cc.disc_mask(pts, np.mean(tower[:128], axis=0)[:2], 15.0)]
    assert np.array_equal(_bits(samples[1]), cc.bits(want))


# ---- 7. capture ------------------------------------------------------------------------------------------------------------------
def test_capture_and_replay_on_refilled_scan_and_regions(hip_device):
    n, K = 2 * _hip.crops_chunk_points() + 300, 6
    cases = [cc.random_case(n, K, seed=s) for s in (41, 42)]
    capacity = max(int(cc.crop_oracle(*c)[0][-1]) for c in cases) + 10
    d_pts, d_lab = _dev(cases[0][0], hip_device, torch.float64), _dev(cases[0][1], hip_device, torch.float64)
    d_reg, d_kinds = _dev(cases[0][2], hip_device, torch.float64), _dev(cases[0][3], hip_device, torch.int32)
    sna.crop_regions(d_pts, d_reg, d_kinds, d_lab, capacity=capacity)       # (an eager call first: kernels are loaded)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        crops = sna.crop_regions(d_pts, d_reg, d_kinds, d_lab, capacity=capacity)
    for pts, labels, regions, kinds in (cases[0], cases[1], cases[0]):
        d_pts.copy_(torch.from_numpy(pts))
        d_lab.copy_(torch.from_numpy(labels))
        d_reg.copy_(torch.from_numpy(regions))
        d_kinds.copy_(torch.from_numpy(kinds))
        graph.replay()
        torch.cuda.synchronize()
        offsets, rows, lab, src = cc.crop_oracle(pts, labels, regions, kinds)
        total = int(offsets[-1])
        assert np.array_equal(crops.offsets.cpu().numpy(), offsets)
        assert np.array_equal(_bits(crops.pts[:total]), cc.bits(rows)) and np.array_equal(_bits(crops.labels[:total]), cc.bits(lab))
        assert np.array_equal(crops.src[:total].cpu().numpy(), src)
    assert not np.array_equal(cc.crop_oracle(*cases[0])[0], cc.crop_oracle(*cases[1])[0])


# ---- 8. byte offsets past 2^32 ---------------------------------------------------------------------------------------------------
def test_byte_offsets_past_4_gib(hip_device):
    free, _ = torch.cuda.mem_get_info()
    if free < 16 * 2 ** 30:
        pytest.skip(f"needs 16 GiB of free device memory for a 4.3 GB scan and its reference (free: {free / 2 ** 30:.1f} GiB)")
    n = 180_000_000
    pts = torch.rand((n, 3), dtype=torch.float64, device=hip_device)
    pts[:, 0] = torch.arange(n, dtype=torch.float64, device=hip_device) * 1e-3       # x rises with the index
    labels = torch.arange(n, dtype=torch.float64, device=hip_device)
    cx = (n - 300_000) * 1e-3
    regions = torch.tensor([[cx, 0.5, 100.0, 0.0], [5.0, 0.25, 60.0, 0.75]], dtype=torch.float64, device=hip_device)
    kinds = torch.tensor([0, 1], dtype=torch.int32, device=hip_device)
    crops = sna.crop_regions(pts, regions, kinds, labels)
    # the torch-on-device formulation: separate kernels per operation, so nothing is contracted
    x, y = pts[:, 0].contiguous(), pts[:, 1].contiguous()
    dx, dy = x - cx, y - 0.5
    disc = torch.add(dx * dx, dy * dy) <= 100.0 * 100.0
    del dx, dy
    box = (x >= 5.0) & (x <= 60.0) & (y >= 0.25) & (y <= 0.75)
    del x, y
    want_src = torch.cat([torch.nonzero(disc).reshape(-1), torch.nonzero(box).reshape(-1)])
    assert crops.offsets.tolist() == [0, int(disc.sum()), int(disc.sum()) + int(box.sum())]
    del disc, box
    assert torch.equal(crops.src, want_src)
    assert int(crops.src[0]) * 24 > 2 ** 32 and 100_000 < crops.offsets[1] < 250_000 and crops.offsets[2] - crops.offsets[1] > 10_000
    assert torch.equal(crops.pts.view(torch.int64), pts.index_select(0, want_src).view(torch.int64))
    assert torch.equal(crops.labels, want_src.to(torch.float64))
    del pts, labels, crops, want_src
    torch.cuda.empty_cache()


# ---- 9. end to end -----------------------------------------------------------------------------------------------------------------
def test_whole_scan_inference_loop(hip_device, golden_dir):
    a = np.load(os.path.join(golden_dir, "ts40k_sample575_subset.npy"))
    m = a.shape[0] // 3
    tiles, labels = [], []
    for j in range(3):
        t = np.ascontiguousarray(a[j * m:(j + 1) * m, :3])
        t[:, 0] += 1000.0 * j
        tiles.append(t)
        labels.append(np.ascontiguousarray(a[j * m:(j + 1) * m, 3]))
    n = 3 * m + 1
    scan, scan_lab = np.empty((n, 3)), np.empty(n)
    for j in range(3):
        scan[j:3 * m:3], scan_lab[j:3 * m:3] = tiles[j], labels[j]
    scan[-1], scan_lab[-1] = [tiles[0][:, 0].min() - 5000.0, tiles[0][0, 1], tiles[0][0, 2]], 0.0      # in no box
    boxes = np.array([[t[:, 0].min(), t[:, 1].min(), t[:, 0].max(), t[:, 1].max()] for t in tiles])
    crops = _crop(hip_device, scan, scan_lab, boxes, np.ones(3, dtype=np.int32))
    batch, kept = crops.point_batch()
    assert kept == [0, 1, 2]
    w_pts, w_lab, w_off, w_sizes = sna.pack_csr(tiles, labels)
    assert batch.sizes == w_sizes and np.array_equal(batch.offsets.cpu().numpy(), w_off)
    assert np.array_equal(_bits(batch.pts), cc.bits(w_pts)) and np.array_equal(_bits(batch.labels), cc.bits(w_lab))

    torch.manual_seed(0)
    model = sna.SceneNet({"cy": 2, "cone": 1, "neg": 1}, (9, 9, 9)).to(hip_device)
    pipe = sna.ScenePipeline(model, (32, 32, 32), keep_labels=[15], per_point=True)
    original = sna.PointBatch.from_tiles(tiles, labels, device=hip_device)
    with torch.no_grad():
        out_c, pp_c = pipe(batch)
        out_o, pp_o = pipe(original)
    assert torch.equal(out_c, out_o) and torch.equal(pp_c, pp_o) and pp_o.shape == (1, 3 * m)
    merged = sna.merge_to_scan(pp_c[0], crops.src_rows(), n, fill=-1.0)
    want = torch.full((n,), -1.0, dtype=pp_o.dtype, device=hip_device)
    for j in range(3):
        want[j:3 * m:3] = pp_o[0, j * m:(j + 1) * m]
    assert torch.equal(merged, want) and float(merged[-1]) == -1.0
    # where tiles overlap, a point reads the largest of its predictions
    twice = sna.merge_to_scan(torch.cat([pp_c[0], pp_c[0] - 0.5]), torch.cat([crops.src_rows()] * 2), n, fill=-1.0)
    assert torch.equal(twice, want)


def test_lattice_regions_on_the_device(hip_device):
    regions, kinds = sna.lattice_regions((100.0, 200.0), (170.0, 265.0), 30.0, overlap=2.5, device=hip_device)
    assert regions.is_cuda and regions.dtype == torch.float64 and kinds.dtype == torch.int32
    assert np.array_equal(regions.cpu().numpy(), lattice_boxes((100.0, 200.0), (170.0, 265.0), 30.0, 2.5))
    assert kinds.cpu().tolist() == [1] * 9
    rng = np.random.default_rng(9)
    pts = np.column_stack([rng.uniform(100, 170, 5000), rng.uniform(200, 265, 5000), rng.uniform(0, 9, 5000)])
    crops = sna.crop_regions(torch.from_numpy(pts).to(hip_device), regions, kinds)
    seen = np.zeros(5000, dtype=int)
    np.add.at(seen, crops.src.cpu().numpy(), 1)
    assert seen.min() >= 1 and seen.max() <= 4
