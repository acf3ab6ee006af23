"""Region census on the device (K12: sn_crop_census, scene_net_amd.census) against the numpy oracle of census_cases --
crops_cases.region_mask for membership, then len, np.isnan, min / max and the literal range test -- and the three sample
builders against numpy restatements of the reference's code.  Every comparison is exact: integers as they are, fp64 as
int64 views.  Every raw call runs on sentinel-filled outputs with guard words on both sides and a workspace full of junk."""
import os

import numpy as np
import pytest
import torch

import scene_net_amd as sna
from scene_net_amd import _hip

import census_cases as cs
import crops_cases as cc

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


def _guarded(words, dev, extra=0):
    """(whole buffer, the `words` int64 words inside it) -- GUARD sentinel words on both sides, the inside sentinel too;
    extra = 1 moves the inside by one word (an address that is 8 but not 16 bytes aligned)"""
    buf = torch.full((words + 2 * GUARD + extra,), SENTINEL, dtype=torch.int64, device=dev)
    return buf, buf[GUARD + extra:GUARD + extra + words]


def _raw(dev, pts, labels, regions, kinds, watch, offset_by_one=False):
    """sn_crop_census on guarded outputs and a junk workspace -> (counts [K, 2 + C] i64, label_range bits [K,2] i64 | None)"""
    n, K = pts.shape[0], regions.shape[0]
    C = 0 if watch is None else watch.shape[0]
    d_pts, d_lab = _dev(pts, dev, torch.float64, offset_by_one), _dev(labels, dev, torch.float64, offset_by_one)
    d_reg, d_kinds = _dev(regions, dev, torch.float64, offset_by_one), _dev(kinds, dev, torch.int32, offset_by_one)
    d_watch = _dev(watch, dev, torch.float64, offset_by_one) if C else None
    extra = 1 if offset_by_one else 0
    ws_buf, ws = _guarded(_hip.crop_census_ws_bytes(n, K, C) // 8, dev, extra)
    c_buf, counts = _guarded(K * (2 + C), dev, extra)
    r_buf, rng = _guarded(2 * K, dev, extra)
    _hip.crop_census(d_pts, d_lab, d_reg, d_kinds, d_watch, ws, counts, None if labels is None else rng.view(torch.float64))
    torch.cuda.synchronize()
    for name, buf, inside in (("ws", ws_buf, ws), ("counts", c_buf, counts), ("label_range", r_buf, rng)):
        b = buf.cpu().numpy()
        lo = GUARD + extra
        assert np.all(b[:lo] == SENTINEL) and np.all(b[lo + inside.numel():] == SENTINEL), f"{name}: guard words were written"
    if labels is None:
        assert np.all(rng.cpu().numpy() == SENTINEL), "label_range is not written without labels"
    return counts.cpu().numpy().reshape(K, 2 + C), (None if labels is None else rng.cpu().numpy().reshape(K, 2))


def _assert_equals_oracle(got, want, C=None, what=""):
    """want: the oracle's (counts, range) for ALL 16 watch rows or exactly those asked for; C: the leading rows asked for"""
    counts, rng = got
    w_counts, w_rng = want
    if C is not None:
        w_counts = w_counts[:, :2 + C]
    assert np.array_equal(counts, w_counts), f"{what}: counts"
    if rng is None:
        assert np.all(counts[:, 1] == 0), f"{what}: n_nan is 0 without labels"
    else:
        assert np.array_equal(rng, cc.bits(w_rng)), f"{what}: label_range"


# ---- 1. seams ----------------------------------------------------------------------------------------------------------
def _seam_sizes():
    c = _hip.census_chunk_points()
    return [1, c - 1, c, c + 1, 3 * c + 17]


SEAM_K = (1, 63, 64, 65, 130)


def _invalid_kinds(kinds):
    out = kinds.copy()
    out[::5], out[3::7], out[4::11] = 2, -1, 1 << 30
    return out


@pytest.mark.parametrize("which", range(5))
def test_seams_of_chunks_region_tiles_and_watch_counts(hip_device, which):
    n = _seam_sizes()[which]
    pts, _, regions, kinds = cc.random_case(n, max(SEAM_K), seed=500 + which)
    labels = cs.odd_labels(n, 600 + which)
    watch = cs.watch_rows(16)
    members = 0
    for j, K in enumerate(SEAM_K):
        # kinds: null (all discs), mixed, mixed with values that are neither disc nor box
        use = (None, kinds[:K], _invalid_kinds(kinds[:K]))[(which + j) % 3]
        want = cs.census_oracle(pts, labels, regions[:K], use, watch)
        want_plain = (np.column_stack([want[0][:, :1], np.zeros((K, 1), dtype=np.int64)]), None)
        off1 = bool((which + j) % 2)
        for C in (0, 1, 16):
            got = _raw(hip_device, pts, labels, regions[:K], use, watch[:C] if C else None, off1)
            _assert_equals_oracle(got, want, C, f"n={n} K={K} C={C} offset={off1}")
        _assert_equals_oracle(_raw(hip_device, pts, None, regions[:K], use, None, not off1), want_plain, None,
                              f"n={n} K={K} without labels")
        members += int(want[0][:, 0].sum())
    assert members > 0


def test_python_layer_with_and_without_labels(hip_device):
    pts, _, regions, kinds = cc.random_case(2500, 40, seed=7)
    labels = cs.odd_labels(2500, 8)
    watch = cs.watch_rows(3)
    d = lambda a, t=torch.float64: _dev(a, hip_device, t)   # noqa: E731
    counts, rng = cs.census_oracle(pts, labels, regions, kinds, watch)
    c = sna.region_census(d(pts), d(regions), d(kinds, torch.int32), d(labels), watch)
    assert np.array_equal(c.counts.cpu().numpy(), counts) and np.array_equal(c.n.cpu().numpy(), counts[:, 0])
    assert np.array_equal(c.n_nan.cpu().numpy(), counts[:, 1]) and np.array_equal(c.watch_counts.cpu().numpy(), counts[:, 2:])
    assert np.array_equal(cc.bits(c.label_min.cpu().numpy()), cc.bits(rng[:, 0]))
    assert np.array_equal(cc.bits(c.label_max.cpu().numpy()), cc.bits(rng[:, 1]))
    want = [cs.distinct_ge2(counts[k, 0], counts[k, 1], rng[k, 0], rng[k, 1]) for k in range(40)]
    got = c.distinct_ge2()
    assert got.is_cuda and got.dtype == torch.bool and got.cpu().tolist() == want and any(want)
    assert bool(sna.scan_has_class(c, 0)) is bool(counts[:, 2].sum() > 0)
    # a device tensor as watch, and no labels: the range is (+inf, -inf), n_nan 0, no watch columns
    c1 = sna.region_census(d(pts), d(regions), d(kinds, torch.int32), d(labels), d(watch))
    assert torch.equal(c1.counts, c.counts)
    c0 = sna.region_census(d(pts), d(regions), d(kinds, torch.int32))
    assert np.array_equal(c0.n.cpu().numpy(), counts[:, 0]) and c0.watch_counts.shape == (40, 0) and int(c0.n_nan.sum()) == 0
    assert torch.all(c0.label_min == float("inf")) and torch.all(c0.label_max == float("-inf")) and not bool(c0.distinct_ge2().any())
    with pytest.raises(ValueError):
        sna.region_census(d(pts), d(regions), None, None, watch)
    # the scan-level gate
    assert bool(sna.scan_has_class(d(labels), 80.0)) is True and bool(sna.scan_has_class(d(labels), 81.0)) is False
    assert bool(sna.scan_has_class(d(np.array([np.nan, 2.0])), 15)) is False


# ---- 2. regions ----------------------------------------------------------------------------------------------------------
def test_overlapping_repeated_and_empty_regions(hip_device):
    pts, _, _, _ = cc.random_case(3000, 1, seed=21)
    labels = cs.odd_labels(3000, 22)
    c = cc.ORIGIN[:2] + 30.0
    regions = np.array([[c[0], c[1], 12.0, 0.0], [c[0], c[1], 12.0, 0.0], [c[0], c[1], 5.0, 0.0], [c[0], c[1], 40.0, 0.0],
                        [-np.inf, -np.inf, np.inf, np.inf], [0.0, 0.0, 10.0, 0.0], [c[0], c[1], np.nan, 0.0],
                        [c[0] + 5, c[1] - 5, c[0] - 5, c[1] + 5], [c[0], c[1], np.inf, 0.0]])
    kinds = np.array([0, 0, 0, 0, 1, 0, 0, 1, 7], dtype=np.int32)
    watch = cs.watch_rows(16)
    want = cs.census_oracle(pts, labels, regions, kinds, watch)
    got = _raw(hip_device, pts, labels, regions, kinds, watch)
    _assert_equals_oracle(got, want, 16, "overlap")
    counts, rng = got
    assert np.array_equal(counts[0], counts[1]) and np.array_equal(rng[0], rng[1]) and 0 < counts[2, 0] < counts[0, 0] < counts[3, 0]
    assert counts[4, 0] == 3000 and counts[4, 1] == np.isnan(labels).sum() > 0
    assert np.all(counts[5:] == 0), "regions without a member count nothing"
    assert np.array_equal(rng[5:], np.tile(cc.bits(np.array([np.inf, -np.inf])), (4, 1)))
    # a watch range with a NaN bound, a reversed one and (NaN, NaN) match nothing, though the labels hold 80 and NaN
    assert np.all(counts[:, 2 + 4] == 0) and np.all(counts[:, 2 + 5] == 0) and np.all(counts[:, 2 + 6] == 0) and np.all(counts[:, 2 + 13] == 0)
    assert counts[4, 2 + 2] == 3000 - counts[4, 1], "(-inf, +inf) holds every label that is not NaN"
    assert counts[4, 2 + 3] == ((labels == 0)).sum() > 0, "(0.0, -0.0) holds both zeros: the test is numeric"
    assert np.array_equal(rng[4], cc.bits(np.array([-np.inf, np.inf])))


def test_a_region_only_the_last_chunk_reaches(hip_device):
    pts, labels, regions, kinds = cs.late_chunk_case(_hip.census_chunk_points())
    watch = cs.watch_rows(16)
    want = cs.census_oracle(pts, labels, regions, kinds, watch)
    assert want[0][0, 0] > 0 and want[0][1, 0] == 0 and want[0][2, 0] == 7
    _assert_equals_oracle(_raw(hip_device, pts, labels, regions, kinds, watch), want, 16, "late chunk")


def test_exact_boundaries_show_in_n(hip_device):
    pts, labels, regions, kinds, claims = cc.boundary_case()
    want = cs.census_oracle(pts, labels, regions, kinds, None)
    got = _raw(hip_device, pts, labels, regions, kinds, None)
    _assert_equals_oracle(got, want, 0, "boundary")
    # each claimed point alone against every region: n says whether it is a member
    for i in sorted({i for _, i, _ in claims}):
        alone, _ = _raw(hip_device, pts[i:i + 1], labels[i:i + 1], regions, kinds, None)
        for k, _, member in (c for c in claims if c[1] == i):
            assert alone[k, 0] == int(member), (k, i, member)
    # labels are the point indices: a region's range names its first and last member
    counts, rng = got
    for k in range(len(regions)):
        idx = np.flatnonzero(cc.region_mask(pts, regions[k], int(kinds[k])))
        span = np.array([idx[0], idx[-1]] if len(idx) else [np.inf, -np.inf], dtype=np.float64)
        assert counts[k, 0] == len(idx) and np.array_equal(rng[k], cc.bits(span))


def test_chunk_reject_keeps_a_point_on_the_rim_of_its_chunk(hip_device):
    pts, labels, regions, kinds, claims = cc.rim_case(_hip.census_chunk_points())
    want = cs.census_oracle(pts, labels, regions, kinds, None)
    got = _raw(hip_device, pts, labels, regions, kinds, None)
    _assert_equals_oracle(got, want, 0, "rim")
    assert got[0][0, 0] == 2 and got[0][1, 0] == 0 and got[0][4, 0] == 2


def test_nonfinite_scan_and_regions(hip_device):
    pts, labels, regions, kinds = cc.nonfinite_case()
    watch = cs.watch_rows(16)
    want = cs.census_oracle(pts, labels, regions, kinds, watch)
    got = _raw(hip_device, pts, labels, regions, kinds, watch)
    _assert_equals_oracle(got, want, 16, "non-finite")
    k = 9       # the box of infinite bounds: every point without a NaN in x or y
    assert got[0][k, 0] == (~np.isnan(pts[:, 0]) & ~np.isnan(pts[:, 1])).sum() and got[0][k, 1] >= 3
    assert np.array_equal(got[1][k], cc.bits(np.array([-np.inf, np.inf])))


def test_signed_zeros_and_denormals_in_the_range(hip_device):
    pts = np.zeros((6, 3))
    pts[:, 0] = np.arange(6)
    labels = np.array([0.0, -0.0, 5e-324, -5e-324, np.nan, 0.0])
    box = lambda a, b: [a - 0.5, -1.0, b + 0.5, 1.0]   # noqa: E731
    regions = np.array([box(0, 1), box(1, 1), box(0, 0), box(0, 3), box(4, 4), box(4, 5), box(2, 2)])
    kinds = np.ones(7, dtype=np.int32)
    counts, rng = _raw(hip_device, pts, labels, regions, kinds, np.array([[-5e-324, 0.0]]))
    z, mz, d, md, inf = 0.0, -0.0, 5e-324, -5e-324, np.inf
    assert np.array_equal(rng, cc.bits(np.array([[mz, z], [mz, mz], [z, z], [md, d], [inf, -inf], [z, z], [d, d]])))
    assert counts.tolist() == [[2, 0, 2], [1, 0, 1], [1, 0, 1], [4, 0, 3], [1, 1, 0], [2, 1, 1], [1, 0, 0]]
    _assert_equals_oracle((counts, rng), cs.census_oracle(pts, labels, regions, kinds, np.array([[-5e-324, 0.0]])), 1, "zeros")


def test_workgroups_that_share_a_shard_of_the_workspace(hip_device):
    """20 workgroups over the 8 shards: counts are added onto slots that already hold a value, a maximum meets one that is
    there, and a region's smallest and largest label arrive from different workgroups of ONE shard.  Once eager on a junk
    workspace, then captured and replayed twice."""
    chunk = _hip.census_chunk_points()
    pts, labels, regions, kinds = cs.shard_case(chunk)
    assert pts.shape[0] == 19 * chunk + 17 >= (2 * cs.SHARDS + 1) * chunk
    watch = cs.watch_rows(16)
    want = cs.census_oracle(pts, labels, regions, kinds, watch)
    per_chunk = np.array([cs.census_oracle(pts[c * chunk:(c + 1) * chunk], None, regions, kinds, None)[0][:, 0] for c in range(20)])
    assert np.all(per_chunk[:, :4] > 0), "the covering box and the three discs hold members in every chunk"
    assert np.flatnonzero(per_chunk[:, 5]).tolist() == [1, 9, 17] and want[0][5].tolist()[:2] == [10, 2]
    assert np.array_equal(cc.bits(want[1][5]), cc.bits(np.array([-1e300, 1e300]))) and want[0][4, 0] == 0
    for off1 in (False, True):
        _assert_equals_oracle(_raw(hip_device, pts, labels, regions, kinds, watch, off1), want, 16, f"shards, offset={off1}")
    _assert_equals_oracle(_raw(hip_device, pts, None, regions, kinds, None), (np.column_stack([want[0][:, :1], 0 * want[0][:, :1]]), None),
                          None, "shards, no labels")
    d_pts, d_lab = _dev(pts, hip_device, torch.float64), _dev(labels, hip_device, torch.float64)
    d_reg, d_kinds = _dev(regions, hip_device, torch.float64), _dev(kinds, hip_device, torch.int32)
    d_watch = _dev(watch, hip_device, torch.float64)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        c = sna.region_census(d_pts, d_reg, d_kinds, d_lab, d_watch)
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(c.counts.cpu().numpy(), want[0])
        assert np.array_equal(cc.bits(c.label_min.cpu().numpy()), cc.bits(want[1][:, 0]))
        assert np.array_equal(cc.bits(c.label_max.cpu().numpy()), cc.bits(want[1][:, 1]))


# ---- 3. the tie to K9 --------------------------------------------------------------------------------------------------------
def test_n_is_the_size_sn_crop_count_reports(hip_device):
    n = 2 * _hip.census_chunk_points() + 77
    for seed, use_kinds in ((31, True), (32, False)):
        pts, labels, regions, kinds = cc.random_case(n, 70, seed=seed)
        kinds = _invalid_kinds(kinds) if use_kinds else None
        d_pts, d_reg = _dev(pts, hip_device, torch.float64), _dev(regions, hip_device, torch.float64)
        d_kinds = _dev(kinds, hip_device, torch.int32)
        ws = torch.empty(_hip.crops_ws_bytes(n, 70) // 8, dtype=torch.int64, device=hip_device)
        offsets = torch.empty(71, dtype=torch.int64, device=hip_device)
        _hip.crop_count(d_pts, d_reg, d_kinds, ws, offsets)
        census = sna.region_census(d_pts, d_reg, d_kinds)
        assert torch.equal(census.n, offsets[1:] - offsets[:-1]) and int(census.n.sum()) > 0


# ---- 4. determinism and capture ------------------------------------------------------------------------------------------------
def test_two_runs_and_a_captured_replay_agree(hip_device):
    n, K = 3 * _hip.census_chunk_points() + 300, 70
    watch = cs.watch_rows(16)
    cases = []
    for s in (41, 42):
        pts, _, regions, kinds = cc.random_case(n, K, seed=s)
        cases.append((pts, cs.odd_labels(n, s + 100), regions, kinds))
    d_pts, d_lab = _dev(cases[0][0], hip_device, torch.float64), _dev(cases[0][1], hip_device, torch.float64)
    d_reg, d_kinds = _dev(cases[0][2], hip_device, torch.float64), _dev(cases[0][3], hip_device, torch.int32)
    d_watch = _dev(watch, hip_device, torch.float64)
    a = sna.region_census(d_pts, d_reg, d_kinds, d_lab, d_watch)
    b = sna.region_census(d_pts, d_reg, d_kinds, d_lab, d_watch)
    assert torch.equal(a.counts, b.counts) and torch.equal(a.label_min.view(torch.int64), b.label_min.view(torch.int64))
    assert torch.equal(a.label_max.view(torch.int64), b.label_max.view(torch.int64))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        c = sna.region_census(d_pts, d_reg, d_kinds, d_lab, d_watch)
        distinct = c.distinct_ge2()
    for pts, labels, regions, kinds in (cases[0], cases[1], cases[0]):
        d_pts.copy_(torch.from_numpy(pts))
        d_lab.copy_(torch.from_numpy(labels))
        d_reg.copy_(torch.from_numpy(regions))
        d_kinds.copy_(torch.from_numpy(kinds))
        graph.replay()
        torch.cuda.synchronize()
        counts, rng = cs.census_oracle(pts, labels, regions, kinds, watch)
        assert np.array_equal(c.counts.cpu().numpy(), counts)
        assert np.array_equal(cc.bits(c.label_min.cpu().numpy()), cc.bits(rng[:, 0]))
        assert np.array_equal(cc.bits(c.label_max.cpu().numpy()), cc.bits(rng[:, 1]))
        assert distinct.cpu().tolist() == [cs.distinct_ge2(counts[k, 0], counts[k, 1], rng[k, 0], rng[k, 1]) for k in range(K)]
    assert not np.array_equal(cs.census_oracle(*cases[0], watch)[0], cs.census_oracle(*cases[1], watch)[0])


# ---- 5. accept, then crop --------------------------------------------------------------------------------------------------------
def _accept_oracle(pts, labels, regions, kinds):
    counts, rng = cs.census_oracle(pts, labels, regions, kinds, sna.watch_trunc([15]).numpy())
    distinct = np.array([cs.distinct_ge2(counts[k, 0], counts[k, 1], rng[k, 0], rng[k, 1]) for k in range(len(regions))])
    return (counts[:, 0] > 300) & distinct & (counts[:, 2] == 0)


def test_crop_accepted_with_a_capacity_reads_nothing_back(hip_device):
    """census, predicate and K9 inside ONE graph capture: a host read or a synchronisation would end the capture with an
    error.  Replayed on a second scan."""
    n, K = 2 * _hip.census_chunk_points() + 300, 12
    cases = []
    for s in (51, 52):
        pts, _, regions, kinds = cc.random_case(n, K, seed=s)
        labels = np.random.default_rng(s).choice(np.array([0.0, 2.0, 15.5, 16.0]), n, p=[0.5, 0.4985, 0.0015, 0.0])
        cases.append((pts, labels, regions, kinds))
    wants = [_accept_oracle(*c) for c in cases]
    assert all(w.any() and not w.all() for w in wants) and not np.array_equal(wants[0], wants[1])
    capacity = max(int(cc.crop_oracle(*c)[0][-1]) for c in cases)
    d_pts, d_lab = _dev(cases[0][0], hip_device, torch.float64), _dev(cases[0][1], hip_device, torch.float64)
    d_reg, d_kinds = _dev(cases[0][2], hip_device, torch.float64), _dev(cases[0][3], hip_device, torch.int32)
    d_watch = sna.watch_trunc([15], device=hip_device)
    predicate = lambda c: (c.n > 300) & c.distinct_ge2() & (c.watch_counts[:, 0] == 0)   # noqa: E731
    sna.crop_accepted(d_pts, d_reg, d_kinds, d_lab, predicate, capacity=capacity, watch=d_watch)      # (eager first: kernels are loaded)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        crops, accept = sna.crop_accepted(d_pts, d_reg, d_kinds, d_lab, predicate, capacity=capacity, watch=d_watch)
    for (pts, labels, regions, kinds), want in zip(cases, wants):
        d_pts.copy_(torch.from_numpy(pts))
        d_lab.copy_(torch.from_numpy(labels))
        d_reg.copy_(torch.from_numpy(regions))
        d_kinds.copy_(torch.from_numpy(kinds))
        graph.replay()
        torch.cuda.synchronize()
        assert accept.cpu().numpy().tolist() == want.tolist()
        edited = np.where(want, kinds, -1).astype(np.int32)
        assert np.array_equal(crops.kinds.cpu().numpy(), edited)
        offsets, rows, lab, src = cc.crop_oracle(pts, labels, regions, edited)
        total = int(offsets[-1])
        assert np.array_equal(crops.offsets.cpu().numpy(), offsets) and 0 < total <= capacity
        assert np.array_equal(crops.pts[:total].cpu().contiguous().view(torch.int64).numpy(), cc.bits(rows))
        assert np.array_equal(crops.labels[:total].cpu().view(torch.int64).numpy(), cc.bits(lab))
        assert np.array_equal(crops.src[:total].cpu().numpy(), src)


def test_accept_kinds(hip_device):
    accept = torch.tensor([True, False, True, False], device=hip_device)
    assert sna.accept_kinds(None, accept).cpu().tolist() == [0, -1, 0, -1]
    kinds = torch.tensor([1, 1, 0, 5], dtype=torch.int32, device=hip_device)
    out = sna.accept_kinds(kinds, accept)
    assert out.dtype == torch.int32 and out.is_cuda and out.cpu().tolist() == [1, -1, 0, -1]
    # a mask given as it is, and all regions rejected: every tile is empty
    pts, labels, regions, _ = cc.random_case(700, 4, seed=61)
    d = lambda a, t=torch.float64: _dev(a, hip_device, t)   # noqa: E731
    crops, got = sna.crop_accepted(d(pts), d(regions), kinds, d(labels), torch.zeros(4, dtype=torch.bool, device=hip_device))
    assert crops.offsets.cpu().tolist() == [0] * 5 and got.cpu().tolist() == [False] * 4


# ---- 6. the mirrors, end to end ------------------------------------------------------------------------------------------------
def _assert_samples_equal(got, want, what):
    assert len(got) == len(want), what
    for g, w in zip(got, want):
        assert g.is_cuda and g.dtype == torch.float64 and tuple(g.shape) == w.shape and w.shape[1] == 4, what
        assert np.array_equal(g.cpu().contiguous().view(torch.int64).numpy(), cc.bits(w)), what


def test_ground_samples_on_the_golden_scan(hip_device, golden_dir):
    g = np.load(os.path.join(golden_dir, "scan_census.npz"))
    scan = g["scan"]
    xyz, classes = np.ascontiguousarray(scan[:, :3]), np.ascontiguousarray(scan[:, 3])
    want, masks = cs.ground_samples_restated(xyz, classes)
    d_xyz, d_cls = _dev(xyz, hip_device, torch.float64), _dev(classes, hip_device, torch.float64)
    got = sna.crop_ground_samples(d_xyz, d_cls)
    assert len(got) == int(g["n_samples"][0]) == 4
    _assert_samples_equal(got, want, "ground samples")
    for i, s in enumerate(got):       # and straight against what the reference recorded
        m = np.unpackbits(g[f"sample_{i}_bits"])[:len(scan)].astype(bool)
        assert np.array_equal(s[:, :3].cpu().contiguous().view(torch.int64).numpy(), cc.bits(xyz[m]))
        assert np.array_equal(s[:, 3].cpu().numpy(), g[f"sample_{i}_class"].astype(np.float64))
    # nothing is accepted: a single class everywhere; too short a scan: no slab at all
    assert sna.crop_ground_samples(d_xyz, torch.full_like(d_cls, 2.0)) == []
    assert cs.ground_samples_restated(xyz, np.full_like(classes, 2.0))[0] == []
    short = d_xyz.clone()
    short[:, 0] = d_xyz[:, 0].min() + (d_xyz[:, 0] - d_xyz[:, 0].min()) / 16.0
    assert sna.crop_ground_samples(short, d_cls) == [] and cs.ground_samples_restated(short.cpu().numpy(), classes)[0] == []
    # step == 1: the single slab starts at xmin
    rng = np.random.default_rng(71)
    small = np.column_stack([cc.ORIGIN[0] + np.round(rng.uniform(0, 1.5, 700) * 1024) / 1024, cc.ORIGIN[1] + rng.random(700),
                             cc.ORIGIN[2] + rng.random(700)])
    small[0, 0], small[1, 0] = cc.ORIGIN[0], cc.ORIGIN[0] + 150.0
    small_cls = rng.choice(np.array([0.0, 2.5]), 700)
    w1, _ = cs.ground_samples_restated(small, small_cls)
    assert len(w1) == 1 and 300 < len(w1[0]) < 699
    _assert_samples_equal(sna.crop_ground_samples(_dev(small, hip_device, torch.float64), _dev(small_cls, hip_device, torch.float64)),
                          w1, "one slab")


@pytest.mark.parametrize("axis", range(3))
def test_pole_builders_on_a_kitti_shaped_scan(hip_device, axis):
    xyz, gt = cs.kitti_scan(axis)
    d_xyz, d_gt = _dev(xyz, hip_device, torch.float64), _dev(gt, hip_device, torch.float64)
    want = cs.pole_slabs_restated(xyz, gt)
    assert len(want) == 2
    _assert_samples_equal(sna.crop_pole_slabs(d_xyz, d_gt), want, f"pole slabs, axis {axis}")
    want = cs.pole_radius_restated(xyz, gt)
    assert len(want) == 2
    _assert_samples_equal(sna.pole_radius_samples(d_xyz, d_gt), want, f"pole discs, axis {axis}")
    # a higher bar rejects the discs and slabs that a lower one takes
    want = cs.pole_slabs_restated(xyz, gt)
    got = sna.crop_pole_slabs(d_xyz, d_gt, min_poles=17)
    assert len(got) == 1 and np.array_equal(got[0].cpu().contiguous().view(torch.int64).numpy(), cc.bits(want[1]))


def test_pole_builders_accept_nothing_without_poles(hip_device):
    xyz, gt = cs.kitti_scan(1, poles=False)
    d_xyz, d_gt = _dev(xyz, hip_device, torch.float64), _dev(gt, hip_device, torch.float64)
    assert sna.crop_pole_slabs(d_xyz, d_gt) == [] and cs.pole_slabs_restated(xyz, gt) == []
    assert sna.pole_radius_samples(d_xyz, d_gt) == [] and cs.pole_radius_restated(xyz, gt) == []
    assert bool(sna.scan_has_class(d_gt, 80)) is False
