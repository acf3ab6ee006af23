"""Region census (K12), the part that needs no GPU: the restated crop_ground_samples against the reference's recorded
samples, the distinct-classes predicate against np.unique, the truncation ranges against astype(int), the slab rows, and
the argument checks of the C entry."""
import ctypes
import os

import numpy as np
import pytest
import torch

import scene_net_amd as sna
from scene_net_amd import _hip
from scene_net_amd.census import slab_rows

import census_cases as cs
import crops_cases as cc


# ---- 1. the golden scan ------------------------------------------------------------------------------------------------
def test_restated_ground_samples_equal_the_reference_bits(golden_dir):
    g = np.load(os.path.join(golden_dir, "scan_census.npz"))
    scan = g["scan"]
    assert scan.shape[0] <= 8000 and scan.shape[1] == 4
    xyz, classes = np.ascontiguousarray(scan[:, :3]), np.ascontiguousarray(scan[:, 3])
    samples, masks = cs.ground_samples_restated(xyz, classes)
    assert len(samples) == int(g["n_samples"][0]) >= 3
    for i, (s, m) in enumerate(zip(samples, masks)):
        assert np.array_equal(np.packbits(m), g[f"sample_{i}_bits"]), i
        assert np.array_equal(s[:, 3], g[f"sample_{i}_class"].astype(np.float64)), i
        assert np.array_equal(cc.bits(s[:, :3]), cc.bits(xyz[m])), i
    # the scan holds one slab for every cause of rejection, seen through the census oracle
    lo, hi = xyz[:, 0].min(), xyz[:, 0].max()
    step = int((hi - lo) / 100)
    assert step == 9
    rows = slab_rows(np.linspace(lo, hi, step), step, 0)
    counts, rng = cs.census_oracle(xyz, classes, rows, np.ones(step, dtype=np.int32), sna.watch_trunc([cs.TOWER]).numpy())
    distinct = [cs.distinct_ge2(counts[k, 0], counts[k, 1], rng[k, 0], rng[k, 1]) for k in range(step)]
    accept = [bool(counts[k, 0] > 300 and distinct[k] and counts[k, 2] == 0) for k in range(step)]
    assert [k for k in range(step) if accept[k]] == [0, 1, 2, 4] and [int(counts[k, 0]) for k in (0, 1, 2, 4)] == [len(s) for s in samples]
    assert counts[3, 0] > 300 and distinct[3] and counts[3, 2] == 1, "rejected for its tower point alone (15.7)"
    assert counts[5, 0] > 300 and not distinct[5] and counts[5, 2] == 0, "rejected for its single class alone"
    assert counts[6, 0] == 300 and distinct[6] and counts[6, 2] == 0, "rejected for holding exactly 300 points"
    assert counts[8, 0] == 1 and counts[7, 0] == 0, "the last slab holds the xmax point alone"
    for k, m in zip((0, 1, 2, 4), masks):
        assert np.array_equal(cc.region_mask(xyz, rows[k], cc.BOX), m)


# ---- 2. distinct classes -----------------------------------------------------------------------------------------------
def _label_sets():
    rng = np.random.default_rng(5)
    nan, inf = np.nan, np.inf
    sets = [[2.0], [2.0, 2.0, 2.0], [0.0, -0.0], [-0.0, -0.0], [0.0, -0.0, 0.0, 1.0], [nan], [nan, nan, nan], [nan, 2.0],
            [nan, nan, 2.0, 2.0], [nan, 0.0, -0.0], [inf, inf], [inf, -inf], [5e-324, 0.0], [5e-324, -5e-324], [nan, inf],
            [15.0, np.nextafter(15.0, 16.0)], [-0.0, nan, nan]]
    for _ in range(200):
        m = int(rng.integers(1, 9))
        sets.append(rng.choice(np.array([nan, 0.0, -0.0, 2.0, 15.0, inf, -inf, 5e-324]), m).tolist())
    return [np.array(s, dtype=np.float64) for s in sets]


def test_distinct_ge2_is_np_unique():
    seen = set()
    for l in _label_sets():
        pts = np.zeros((len(l), 3))
        counts, rng = cs.census_oracle(pts, l, np.array([[-np.inf, -np.inf, np.inf, np.inf]]), np.array([1], dtype=np.int32), None)
        got = cs.distinct_ge2(counts[0, 0], counts[0, 1], rng[0, 0], rng[0, 1])
        want = len(np.unique(l)) >= 2
        assert got is bool(want), l
        seen.add(got)
        # and the tensor form of the same predicate
        c = sna.RegionCensus(torch.tensor([counts[0, 0]]), torch.tensor([counts[0, 1]]), torch.tensor([rng[0, 0]]),
                             torch.tensor([rng[0, 1]]), torch.zeros((1, 0), dtype=torch.int64), torch.from_numpy(counts))
        assert bool(c.distinct_ge2()[0]) is got
    assert seen == {True, False}


def test_min_max_order_puts_minus_zero_below_plus_zero():
    one = lambda l: cs.census_oracle(np.zeros((len(l), 3)), np.array(l), np.array([[-np.inf, -np.inf, np.inf, np.inf]]),  # noqa: E731
                                     np.array([1], dtype=np.int32), None)[1][0]
    assert cc.bits(one([0.0, -0.0])).tolist() == cc.bits(np.array([-0.0, 0.0])).tolist()
    assert cc.bits(one([0.0, 0.0])).tolist() == cc.bits(np.array([0.0, 0.0])).tolist()
    assert cc.bits(one([-0.0, np.nan])).tolist() == cc.bits(np.array([-0.0, -0.0])).tolist()
    assert cc.bits(one([np.nan])).tolist() == cc.bits(np.array([np.inf, -np.inf])).tolist()


# ---- 3. truncation ranges ------------------------------------------------------------------------------------------------
def test_watch_trunc_is_astype_int():
    values = [15, 1, 80, 0, -1, -3, 2 ** 20]
    w = sna.watch_trunc(values).numpy()
    assert w.shape == (len(values), 2) and w.dtype == np.float64
    probes = []
    for v in values:
        for edge in (float(v), float(v) + 1.0, float(v) - 1.0):
            probes += [edge, np.nextafter(edge, np.inf), np.nextafter(edge, -np.inf), edge + 0.5, edge - 0.5]
    probes += [0.0, -0.0, 5e-324, -5e-324, 0.999, -0.999]
    l = np.array(probes, dtype=np.float64)
    for c, v in enumerate(values):
        inside = (w[c, 0] <= l) & (l <= w[c, 1])
        assert np.array_equal(inside, l.astype(int) == v), v
        assert inside.any() and not inside.all()
        # `v in l.astype(int)` over any subset is `count > 0`
        for sub in (l[::3], l[1::5], l[inside], l[~inside]):
            assert (v in sub.astype(int)) is bool(((w[c, 0] <= sub) & (sub <= w[c, 1])).sum() > 0)
    assert np.array_equal(sna.watch_trunc([15]).numpy(), [[15.0, np.nextafter(16.0, -np.inf)]])
    assert np.array_equal(sna.watch_trunc([0]).numpy(), [[np.nextafter(-1.0, 0.0), np.nextafter(1.0, 0.0)]])
    assert np.array_equal(sna.watch_equal([80, 2.5]).numpy(), [[80.0, 80.0], [2.5, 2.5]])
    with pytest.raises(ValueError):
        sna.watch_trunc([1.5])


def test_slab_rows():
    r = slab_rows([1.0, 0.1], 0.2, 0)
    assert np.array_equal(r, [[1.0, -np.inf, 1.0 + 0.2, np.inf], [0.1, -np.inf, 0.1 + 0.2, np.inf]])
    r = slab_rows(np.array([5.0]), 3, 1)
    assert np.array_equal(r, [[-np.inf, 5.0, np.inf, 8.0]])
    with pytest.raises(sna.HipLibraryError, match="no CPU path"):
        sna.slab_regions([0.0], 1.0, 0, device="cpu")


# ---- 4. the C entry's argument checks -------------------------------------------------------------------------------------
def test_argument_checks_need_no_gpu():
    lib = _hip.load()
    buf = ctypes.create_string_buffer(256)
    p = ctypes.cast(buf, ctypes.c_void_p)
    big = ctypes.c_size_t(1 << 40)
    off = lambda d: ctypes.c_void_p(p.value + d)   # noqa: E731

    def census(pts=p, labels=p, n=100, regions=p, kinds=p, K=3, watch=p, C=2, ws=p, ws_bytes=big, counts=p, label_range=p):
        return lib.sn_crop_census(pts, labels, n, regions, kinds, K, watch, C, ws, ws_bytes, counts, label_range, None)

    for name in ("pts", "regions", "ws", "counts"):
        assert census(**{name: None}) == -1, name
        assert b"null" in lib.sn_last_error()
    for n in (0, -5):
        assert census(n=n) == -1
    for K in (0, -1):
        assert census(K=K) == -1
    assert census(C=-1) == -1
    assert census(labels=None, label_range=None) == -1 and b"without labels" in lib.sn_last_error()      # C > 0 without labels
    assert census(watch=None) == -1 and b"iff" in lib.sn_last_error()
    assert census(C=0) == -1 and b"iff" in lib.sn_last_error()                                              # watch given with C == 0
    assert census(label_range=None) == -1 and b"iff" in lib.sn_last_error()
    assert census(labels=None, watch=None, C=0) == -1 and b"iff" in lib.sn_last_error()                     # label_range without labels
    need = lib.sn_crop_census_ws_bytes(100, 3, 2)
    assert need == 8 * 8 * 3 * (2 + 4), "eight shards of K rows of C + 4 words"
    assert census(ws_bytes=ctypes.c_size_t(need - 1)) == -1
    assert b"sn_crop_census_ws_bytes" in lib.sn_last_error()
    for name in ("pts", "labels", "regions", "watch", "ws", "counts", "label_range"):
        assert census(**{name: off(4)}) == -1, name
        assert b"aligned" in lib.sn_last_error()
    assert census(kinds=off(2)) == -1
    assert census(K=(1 << 16) + 1) == -2 and census(n=(1 << 36) + 1) == -2 and census(C=_hip.SN_CENSUS_MAX_WATCH + 1) == -2
    assert b"beyond" in lib.sn_last_error()


def test_ws_bytes_and_chunk_points():
    lib = _hip.load()
    c = lib.sn_census_chunk_points()
    assert c == _hip.census_chunk_points() and c >= 64 and c % 64 == 0
    for n, K, C in ((0, 1, 0), (-1, 1, 0), (1, 0, 0), (1, -2, 0), ((1 << 36) + 1, 1, 0), (1, (1 << 16) + 1, 0), (1, 1, -1), (1, 1, 17)):
        assert lib.sn_crop_census_ws_bytes(n, K, C) == 0, (n, K, C)
    assert lib.sn_crop_census_ws_bytes(1 << 36, 1 << 16, 16) == 8 * 8 * (1 << 16) * 20
    assert lib.sn_crop_census_ws_bytes(7, 5, 0) == 8 * 8 * 5 * 4
    with pytest.raises(_hip.HipLibraryError):
        _hip.crop_census_ws_bytes(1, 1, 17)


def test_cpu_tensors_raise():
    pts, regions = torch.zeros(8, 3, dtype=torch.float64), torch.zeros(1, 4, dtype=torch.float64)
    lab = torch.zeros(8, dtype=torch.float64)
    with pytest.raises(sna.HipLibraryError, match="no CPU path"):
        sna.region_census(pts, regions)
    with pytest.raises(sna.HipLibraryError, match="no CPU path"):
        sna.accept_kinds(None, torch.ones(3, dtype=torch.bool))
    with pytest.raises(sna.HipLibraryError, match="no CPU path"):
        sna.crop_accepted(pts, regions, None, lab, torch.ones(1, dtype=torch.bool))
    for mirror in (sna.crop_ground_samples, sna.crop_pole_slabs, sna.pole_radius_samples):
        with pytest.raises(sna.HipLibraryError, match="no CPU path"):
            mirror(pts, lab)
    with pytest.raises(sna.HipLibraryError, match="no CPU path"):
        sna.scan_has_class(lab, 15)


def test_kitti_scans_have_the_shape_their_tests_rely_on():
    for axis in range(3):
        xyz, gt = cs.kitti_scan(axis)
        ext = xyz.max(axis=0) - xyz.min(axis=0)
        assert int(np.argmax(ext)) == axis and int(ext[axis] / 10) == 3
        slabs = cs.pole_slabs_restated(xyz, gt)
        assert len(slabs) == 2 and all(s.shape[1] == 4 for s in slabs)
        discs = cs.pole_radius_restated(xyz, gt)
        assert len(discs) == 2
    xyz, gt = cs.kitti_scan(0, poles=False)
    assert cs.pole_slabs_restated(xyz, gt) == [] and cs.pole_radius_restated(xyz, gt) == []


def test_shard_case_makes_workgroups_meet():
    chunk = _hip.census_chunk_points()
    pts, labels, regions, kinds = cs.shard_case(chunk)
    assert pts.shape[0] == 19 * chunk + 17 and cs.SHARDS == 8
    per_chunk = np.array([cs.census_oracle(pts[c * chunk:(c + 1) * chunk], None, regions, kinds, None)[0][:, 0] for c in range(20)])
    assert np.all(per_chunk[:, :4] > 0) and np.all(per_chunk[:, 4] == 0)
    assert np.flatnonzero(per_chunk[:, 5]).tolist() == [1, 9, 17], "three workgroups of shard 1"
    counts, rng = cs.census_oracle(pts, labels, regions, kinds, None)
    assert counts[5].tolist() == [10, 2] and rng[5].tolist() == [-1e300, 1e300]
    far = np.flatnonzero(cc.region_mask(pts, regions[5], cc.BOX))
    assert labels[far[far // chunk == 9]].min() == -1e300 and labels[far[far // chunk == 1]].max() == 1e300
