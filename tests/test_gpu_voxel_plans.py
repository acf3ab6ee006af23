"""K1's LDS-bitmap kernels at every plan they can pick, on the MI355X: the forks of occ_finalize_kernel's emptiness proof
(a wrong "empty" silently gives a wrong occupancy: the tile skips the exact fallback), the z-slab plans at the LDS limit,
the one-pass kernel's forks away from 64^3 and from aligned buffers, and the counting path's column statistics with more
than one trip along y.  Every case first asserts that sn_voxel_occupancy_plan reports the hand-written plan of
tests/voxel_plan_cases.py -- so the fork it names is the fork that runs -- and then compares bit for bit with numpy:
binning_cases.expected_scatter / expected_occ (the rule np.clip(np.searchsorted(edges, p) - 1, 0, n)) and
oracle/voxel_oracle.py (pyntcloud VoxelGrid.compute, utils/voxelization.py:164-204, 244-300,
utils/pcd_processing.py:305-321).  No tolerance anywhere."""
import ctypes

import numpy as np
import pytest
import torch

import binning_cases as bc
import scene_net_amd as sna
import voxel_plan_cases as pc
from oracle import voxel_oracle as vo
from scene_net_amd import _hip

pytestmark = pytest.mark.gpu

_ids = lambda cases: [c.name for c in cases]   # noqa: E731
_cache = {}


def _off8(a, dev):
    """A copy of the host array `a` (f64) on the device, 8 bytes off a 16-byte boundary."""
    big = torch.zeros(a.size + 1, dtype=torch.float64, device=dev)
    v = big[1:].view(a.shape)
    v.copy_(torch.from_numpy(a))
    assert v.data_ptr() % 16 == 8
    return v


def _batch(tiles, labels, dev, aligned=True):
    """PointBatch of the tiles with points AND labels on 16-byte aligned buffers, or both 8 bytes off."""
    pts, lab = np.concatenate(tiles), np.concatenate(labels)
    if aligned:
        d_pts, d_lab = torch.from_numpy(pts).to(dev), torch.from_numpy(lab).to(dev)
        assert d_pts.data_ptr() % 16 == 0 and d_lab.data_ptr() % 16 == 0
    else:
        d_pts, d_lab = _off8(pts, dev), _off8(lab, dev)
    sizes = tuple(len(t) for t in tiles)
    offsets = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int64, device=dev)
    return sna.PointBatch(d_pts, d_lab, offsets, sizes)


def _bounds_desc(dims, B, host, dev):
    bounds = torch.from_numpy(np.stack([bc.bounds_box(b) for b in range(B)])).to(dev)
    desc = _hip.voxel_desc(bounds, dims, from_bounds=True)
    assert np.array_equal(desc.cpu().numpy(), host), "the device's edge tables differ from numpy's"
    return desc, bounds


def _plan_is(case, planes, B, aligned=True, **kw):
    want = case.plan2 if planes == 2 else case.plan1
    got = _hip.voxel_occupancy_plan(case.dims, planes, B, fused=bool(case.fused), pts_aligned16=aligned,
                                    labels_aligned16=aligned, ws_aligned16=bool(case.ws_aligned), **kw)
    assert (got is None) == (want is None) and (want is None or tuple(got) == tuple(want)), (case.name, planes, got, want)


def _np(t):
    return t[:, 0].cpu().numpy()


# ------------------------------------------------------------------ the forks of the finalize kernel
def _recipes(case):
    """recipe_batch(case) with its expectations, computed once per grid and left unchanged."""
    if case.name not in _cache:
        desc, tiles, labels, names, counts, towers = pc.recipe_batch(case)
        c, t, dropped = bc.expected_scatter(desc, case.dims, tiles, labels)
        assert np.array_equal(c, counts) and np.array_equal(t, towers)
        _cache[case.name] = (desc, tiles, labels, names, c, t, dropped, bc.expected_occ(c) != 0, pc.expected_flags(c))
    return _cache[case.name]


def _check_recipes(run, names, counts, towers, dropped, occ, flags, dt, want_gt, tag):
    """run(exact_fallback) -> (occ, gt_occ, flags, dropped).  With the fallback: the oracle's count > column minimum;
    without: the same flags, and every tile (the flagged ones too) holds count > 0."""
    o, g, f, d = run(True)
    assert o.dtype == dt
    bad = [n for n, a, b in zip(names, f.cpu().tolist(), flags.tolist()) if a != b]
    assert not bad, f"{tag}: flags differ from the oracle's in tiles {bad}"
    assert np.array_equal(d.cpu().numpy(), dropped), (tag, d, dropped)
    got = _np(o) != 0
    bad = [n for b, n in enumerate(names) if not np.array_equal(got[b], occ[b])]
    assert not bad, f"{tag}: occupancy differs from ToFullDense(normalize_xyz(counts)) in tiles {bad}"
    assert (g is None) == (not want_gt)
    if want_gt:
        assert np.array_equal(_np(g) != 0, towers > 0), tag
    o2, g2, f2, d2 = run(False)
    assert f2.cpu().tolist() == flags.tolist() and np.array_equal(d2.cpu().numpy(), dropped), tag
    assert np.array_equal(_np(o2) != 0, counts > 0), tag
    if want_gt:
        assert np.array_equal(_np(g2) != 0, towers > 0), tag


@pytest.mark.parametrize("case", pc.FINALIZE, ids=_ids(pc.FINALIZE))
def test_finalize_forks(hip_device, case):
    """sn_voxel_occupancy, descriptor from bounds, one batch of the tile recipes A-E of tests/voxel_plan_cases.py: full
    tiles (flag up; the fallback's result differs from count > 0), the same with one row emptied at every position where
    the proof changes hands (flag down), with that row holding one point at either end of every word that matters (flag
    up), a tower plane with empty rows (the proof reads plane 0) and a sparse tile between flagged ones.  u8 and f32, with
    and without gt_occ, buffers aligned and 8 bytes off."""
    host, tiles, labels, names, counts, towers, dropped, occ, flags = _recipes(case)
    B = len(tiles)
    desc, _ = _bounds_desc(case.dims, B, host, hip_device)
    for aligned in (True, False):
        batch = _batch(tiles, labels, hip_device, aligned)
        for want_gt in (False, True):
            _plan_is(case, 2 if want_gt else 1, B, aligned)
            for dt in (torch.uint8, torch.float32):
                run = lambda fb: _hip.voxel_occupancy(batch.pts, batch.labels, batch.offsets, desc, case.dims, bc.KEEP,   # noqa: E731
                                                      want_gt_occ=want_gt, out_dtype=dt, exact_fallback=fb)
                _check_recipes(run, names, counts, towers, dropped, occ, flags, dt, want_gt, (case.name, aligned, want_gt, dt))


def _occupancy_raw(batch, desc, dims, want_gt, dt, ws_off_words=1, want_flags=True, fallback=True):
    """sn_voxel_occupancy through ctypes with a workspace that starts `ws_off_words` words into a larger buffer."""
    B = len(batch.sizes)
    nx, ny, nz = dims
    V, dev, planes = nx * ny * nz, batch.pts.device, 2 if want_gt else 1
    n = B * _hip.SN_OCC_PARTS * (planes * (V // 32) + 1)
    big = torch.zeros(n + 4, dtype=torch.int32, device=dev)
    bits = big[ws_off_words:ws_off_words + n]
    assert bits.data_ptr() % 16 == (4 * ws_off_words) % 16
    occ = torch.empty((B, 1, nz, nx, ny), dtype=dt, device=dev)
    gt_occ = torch.empty((B, 1, nz, nx, ny), dtype=dt, device=dev) if want_gt else None
    flags = torch.empty((B,), dtype=torch.int32, device=dev) if want_flags else None
    dropped = torch.empty((B,), dtype=torch.int32, device=dev)
    counts = torch.empty((B, V), dtype=torch.int32, device=dev) if fallback and want_flags else None
    tw = torch.empty((B, V), dtype=torch.int32, device=dev) if counts is not None and want_gt else None
    keep = (ctypes.c_double * len(bc.KEEP))(*bc.KEEP)
    ptr = lambda t: None if t is None else t.data_ptr()   # noqa: E731
    rc = _hip.load().sn_voxel_occupancy(ptr(batch.pts), ptr(batch.labels) if want_gt else None, ptr(batch.offsets), B,
                                        ptr(desc), nx, ny, nz, ctypes.cast(keep, ctypes.c_void_p),
                                        len(bc.KEEP) if want_gt else 0, ptr(bits), ptr(occ), ptr(gt_occ),
                                        _hip.SN_U8 if dt == torch.uint8 else _hip.SN_F32, ptr(flags), ptr(dropped),
                                        ptr(counts), ptr(tw), _hip._stream())
    assert rc == 0, _hip.load().sn_last_error()
    return occ, gt_occ, flags, dropped


@pytest.mark.parametrize("case", pc.UNALIGNED_WS, ids=_ids(pc.UNALIGNED_WS))
def test_finalize_forks_on_a_workspace_that_is_only_word_aligned(hip_device, case):
    """The C entry accepts a bits_ws that is only 4-byte aligned (the kernels store and load it word by word unless it is
    16-byte aligned): the four-words-per-thread loop is then off at shapes where it is otherwise on, and the fused proof
    of rows of 1, 2 and 4 words runs in the word loop.  Same recipes, same expectations; and without `flags` no proof runs
    and every tile holds count > 0."""
    host, tiles, labels, names, counts, towers, dropped, occ, flags = _recipes(case)
    B = len(tiles)
    desc, _ = _bounds_desc(case.dims, B, host, hip_device)
    batch = _batch(tiles, labels, hip_device)
    for want_gt in (False, True):
        _plan_is(case, 2 if want_gt else 1, B)
        for dt in (torch.uint8, torch.float32):
            run = lambda fb: _occupancy_raw(batch, desc, case.dims, want_gt, dt, 1, True, fb)   # noqa: E731
            _check_recipes(run, names, counts, towers, dropped, occ, flags, dt, want_gt, (case.name, want_gt, dt))
    for off in (1, 0):
        assert _hip.voxel_occupancy_plan(case.dims, 1, B, ws_aligned16=not off, want_flags=False).proof == 0
        o, _, f, d = _occupancy_raw(batch, desc, case.dims, False, torch.uint8, off, want_flags=False)
        assert f is None and np.array_equal(d.cpu().numpy(), dropped) and np.array_equal(_np(o) != 0, counts > 0)


# ------------------------------------------------------------------ z-slabs
SLAB_CASES = [c for c in pc.SLABS if c.plan1 is not None]


@pytest.mark.parametrize("case", SLAB_CASES, ids=_ids(SLAB_CASES))
def test_slab_plans(hip_device, case):
    """sn_voxel_occupancy at 1, 2, 4, 8 and 16 z-slabs (16: one workgroup per slab streams the whole tile), a bitmap of
    exactly 64 KiB, an nz that is no power of two: B = 2, a few thousand points per tile with one in the last voxel of
    every slab and the first of the next, points outside the box (dropped: counted once however many slabs see them) and
    the tower plane."""
    B = 2
    for planes in (1, 2):
        host, tiles, labels = pc.slab_batch(case, planes, B)
        desc, _ = _bounds_desc(case.dims, B, host, hip_device)
        counts, towers, dropped = bc.expected_scatter(host, case.dims, tiles, labels)
        assert dropped.min() > 0
        occ, flags = bc.expected_occ(counts) != 0, pc.expected_flags(counts)
        for aligned in (True, False):
            _plan_is(case, planes, B, aligned)
            batch = _batch(tiles, labels, hip_device, aligned)
            o, g, f, d = _hip.voxel_occupancy(batch.pts, batch.labels, batch.offsets, desc, case.dims, bc.KEEP,
                                              want_gt_occ=planes == 2, out_dtype=torch.uint8)
            assert f.cpu().tolist() == flags.tolist() and np.array_equal(d.cpu().numpy(), dropped), (planes, aligned, d)
            assert np.array_equal(_np(o) != 0, occ), (planes, aligned)
            if planes == 2:
                assert np.array_equal(_np(g) != 0, towers > 0), aligned


def test_a_grid_the_slab_rule_refuses(hip_device):
    """(64, 128, 65): V % 32 == 0, but 16640 words fit no power-of-two number of z-slabs that divides nz = 65.  The plan
    query and sn_voxel_occupancy refuse it alike, and voxelize_batch(want_occ=True) takes the counting kernels."""
    case = next(c for c in pc.SLABS if c.plan1 is None)
    dims, B = case.dims, 2
    assert (dims[0] * dims[1] * dims[2]) % 32 == 0
    for planes in (1, 2):
        _plan_is(case, planes, B)
        assert not _hip.occupancy_supported(dims, planes)
    p = (ctypes.c_int32 * 8)()
    assert _hip.load().sn_voxel_occupancy_plan(*dims, 1, B, 0, 0, 1, 1, 1, 1, ctypes.cast(p, ctypes.c_void_p)) == -2
    host, tiles, labels = pc.slab_batch(case, 1, B)
    desc, bounds = _bounds_desc(dims, B, host, hip_device)
    batch = _batch(tiles, labels, hip_device)
    with pytest.raises(sna.HipLibraryError, match=r"\(-2\).*LDS bitmap"):
        _hip.voxel_occupancy(batch.pts, batch.labels, batch.offsets, desc, dims, bc.KEEP)
    counts, towers, dropped = bc.expected_scatter(host, dims, tiles, labels)
    fast = sna.voxelize_batch(batch, dims, bc.KEEP, want_occ=True, want_gt_occ=True, bounds=bounds)
    slow = sna.voxelize_batch(batch, dims, bc.KEEP, want_occ=True, want_gt_occ=True, bounds=bounds, want_counts=True)
    assert fast.counts is not None and np.array_equal(fast.counts.cpu().numpy(), counts)
    for g in (fast, slow):
        assert np.array_equal(g.dropped.cpu().numpy(), dropped)
        assert np.array_equal(_np(g.occ), bc.expected_occ(counts).astype(np.float32))
        assert np.array_equal(_np(g.gt_occ), (towers > 0).astype(np.float32))
    assert torch.equal(fast.occ, slow.occ) and torch.equal(fast.gt_occ, slow.gt_occ)


# ------------------------------------------------------------------ the one-pass kernel
MODES = {"one-pass": dict(voxel_onepass=1), "alone": dict(voxel_onepass=1, voxel_onepass_spin=0),
         "two-kernel": dict(voxel_onepass=0)}


def _own_box_expectation(key, tiles, labels, dims, regular):
    """Per tile: the oracle's counts, towers, descriptor and raw box of a cloud voxelised in its own box; once per key."""
    if key not in _cache:
        per = [pc.own_box_counts(t, dims, l, bc.KEEP, regular) for t, l in zip(tiles, labels)]
        counts, towers = np.stack([p[0] for p in per]), np.stack([p[1] for p in per])
        _cache[key] = (counts, towers, np.stack([p[2] for p in per]), np.stack([p[3] for p in per]),
                       bc.expected_occ(counts) != 0, pc.expected_flags(counts))
    return _cache[key]


def _run_fused_modes(case, batch, want_gt, regular, expect, B, aligned, rider=None):
    """sn_voxel_occupancy_fused in the three forms -- one-pass, one-pass with the exchange's wait at zero (every
    workgroup takes the tile's box from the points alone), two-kernel --, each against the oracle and against the others."""
    counts, towers, desc, bbox, occ, flags = expect
    planes = 2 if want_gt else 1
    want = case.plan2 if want_gt else case.plan1
    outs = {}
    for mode, opts in MODES.items():
        with _hip.options(**opts):
            got = _hip.voxel_occupancy_plan(case.dims, planes, B, fused=True, pts_aligned16=aligned, labels_aligned16=aligned)
            assert tuple(got) == tuple(want if mode != "two-kernel" else want._replace(one_pass=0, parts=16 // want.slabs)), \
                (case.name, mode, got)
            o, g, f, d, dsc, bb = _hip.voxel_occupancy_fused(batch.pts, batch.labels, batch.offsets, case.dims, bool(regular),
                                                             bc.KEEP, want_gt_occ=want_gt, out_dtype=torch.uint8,
                                                             want_bbox=True, bank_rider=rider() if rider else None)
            torch.cuda.synchronize()
        tag = (case.name, mode, aligned, want_gt, regular)
        assert np.array_equal(dsc.cpu().numpy(), desc), f"{tag}: descriptor differs from numpy.linspace"
        assert np.array_equal(bb.cpu().numpy(), bbox), tag
        assert f.cpu().tolist() == flags.tolist() and d.cpu().tolist() == [0] * B, tag
        bad = [b for b in range(B) if not np.array_equal(_np(o)[b] != 0, occ[b])]
        assert not bad, f"{tag}: occupancy differs from the oracle in tiles {bad}"
        if want_gt:
            assert np.array_equal(_np(g) != 0, towers > 0), tag
        outs[mode] = (o, g, f, d, dsc, bb)
    for mode in ("alone", "two-kernel"):
        for a, b in zip(outs["one-pass"], outs[mode]):
            assert (a is None and b is None) or torch.equal(a, b), (case.name, mode)
    assert _hip.device_status()[0] == 0
    return outs


ONEPASS_RAGGED = pc.ONEPASS[:3]


@pytest.mark.parametrize("case", ONEPASS_RAGGED, ids=_ids(ONEPASS_RAGGED))
def test_one_pass_forks(hip_device, case):
    """sn_voxel_occupancy_fused on one ragged batch whose sizes sit on both sides of every edge of the one-pass kernel: 1,
    2 and 3 points, one under / at / over a workgroup part's first pair round, the register budget of 114 688 points - 1,
    exact, + 1, + 3, and 131 073 -- so that a lone first point (aligned form, odd start) and a lone last point each meet
    the surplus stream --, at a 4-word bitmap, a 128-word one and the production grid, buffers aligned and 8 bytes off,
    with and without the tower plane, in the cube (regular = 1) and in the box as it is (regular = 0)."""
    if "onepass" not in _cache:
        _cache["onepass"] = pc.onepass_tiles()
    tiles, labels = _cache["onepass"]
    B = len(tiles)
    for regular in (1, 0):
        expect = _own_box_expectation(("own", case.dims, regular), tiles, labels, case.dims, regular)
        for aligned in (True, False):
            batch = _batch(tiles, labels, hip_device, aligned)
            for want_gt in (False, True):
                _run_fused_modes(case, batch, want_gt, regular, expect, B, aligned)


def test_one_pass_forks_with_a_bank_rider(hip_device):
    """the same batch at 64^3 with K2 riding in the first grid rows (sn_voxel_occupancy_fused_bank), aligned and 8 bytes
    off, in the three forms: the grids are the ones the launch without riders gives, the bank is compute_bank's."""
    case = pc.ONEPASS[2]
    if "onepass" not in _cache:
        _cache["onepass"] = pc.onepass_tiles()
    tiles, labels = _cache["onepass"]
    B = len(tiles)
    model = sna.SceneNet({"cy": 2, "cone": 1, "neg": 1}, (9, 9, 9)).to(hip_device)
    bank = model.compute_bank(hip_device)
    expect = _own_box_expectation(("own", case.dims, 1), tiles, labels, case.dims, 1)
    riders = []

    def rider():
        riders.append(model.bank_rider(hip_device))
        return riders[-1]
    for aligned in (True, False):
        batch = _batch(tiles, labels, hip_device, aligned)
        _run_fused_modes(case, batch, True, 1, expect, B, aligned, rider)
    assert len(riders) == 6
    for r in riders:
        assert torch.equal(r[2], bank) and torch.equal(r[3], riders[0][3])


def test_one_pass_at_the_lds_limit(hip_device):
    """(64, 64, 128): 16384 words, a full 64 KiB bitmap.  One plane is the largest grid the one-pass kernel serves (and the
    two-kernel form in one slab); the tower plane needs two slabs, so the fused entry must take the two-kernel form."""
    case = pc.ONEPASS[3]
    B = 2
    _, tiles, labels = pc.slab_batch(case, 1, B)
    expect = _own_box_expectation(("own", case.dims, 1, "limit"), tiles, labels, case.dims, 1)
    batch = _batch(tiles, labels, hip_device)
    outs = _run_fused_modes(case, batch, False, 1, expect, B, True)
    assert case.plan2.one_pass == 0 and case.plan2.slabs == 2
    for opts in MODES.values():
        with _hip.options(**opts):
            assert tuple(_hip.voxel_occupancy_plan(case.dims, 2, B, fused=True)) == tuple(case.plan2)
    o, g, f, d, dsc, _ = _hip.voxel_occupancy_fused(batch.pts, batch.labels, batch.offsets, case.dims, True, bc.KEEP,
                                                    want_gt_occ=True, out_dtype=torch.uint8)
    assert torch.equal(o, outs["one-pass"][0]) and torch.equal(dsc, outs["one-pass"][4]) and d.cpu().tolist() == [0] * B
    assert np.array_equal(_np(g) != 0, expect[1] > 0)


# ------------------------------------------------------------------ the counting path
@pytest.mark.parametrize("dims", pc.COUNTING_DIMS, ids=["x".join(map(str, d)) for d in pc.COUNTING_DIMS])
def test_counting_path_column_statistics(hip_device, dims):
    """colstats_kernel with ny > 256 (a second trip along y, whose width leaves row lanes idle), ny = 256 exactly and a
    width that does not divide the workgroup: counts, towers, fp64 density and ratio, occ and gt_occ bit for bit --
    through sn_voxel_scatter + sn_voxel_finalize and through voxelize_batch(want_density=True, want_gt=True).  One tile's
    column minima are nonzero in every trip."""
    grids, tgrids = pc.counting_grids(dims)
    B = len(grids)
    host, _ = bc.host_desc("bounds", dims, B)
    desc, bounds = _bounds_desc(dims, B, host, hip_device)
    clouds = [pc.cloud_from_counts(host[b], dims, grids[b], tgrids[b], n_outside=4, seed=b) for b in range(B)]
    tiles, labels = [c[0] for c in clouds], [c[1] for c in clouds]
    counts, towers, dropped = bc.expected_scatter(host, dims, tiles, labels)
    assert np.array_equal(counts, np.stack(grids)) and counts[1].min() >= 1
    density = np.stack([vo.normalize_xyz(c.astype(np.float64)) for c in counts])
    ratio = np.where(counts > 0, towers / np.maximum(counts, 1), 0.0)
    for aligned in (True, False):
        batch = _batch(tiles, labels, hip_device, aligned)
        c, t, d = _hip.voxel_scatter(batch.pts, batch.labels, batch.offsets, desc, dims, bc.KEEP, want_towers=True)
        dens, gt, occ, gt_occ = _hip.voxel_finalize(c, t, want_density=True, want_gt=True, want_occ=True, want_gt_occ=True)
        g = sna.voxelize_batch(batch, dims, bc.KEEP, want_density=True, want_gt=True, want_occ=True, want_gt_occ=True,
                               bounds=bounds)
        for cc, tt, dd, de, gg, oo, go in ((c, t, d, dens, gt, occ, gt_occ),
                                           (g.counts, g.towers, g.dropped, g.density, g.gt, g.occ, g.gt_occ)):
            assert np.array_equal(cc.cpu().numpy(), counts) and np.array_equal(tt.cpu().numpy(), towers)
            assert np.array_equal(dd.cpu().numpy(), dropped)
            assert np.array_equal(_np(de), density), "fp64 density differs from normalize_xyz"
            assert np.array_equal(_np(gg), ratio)
            assert np.array_equal(_np(oo), (density > 0).astype(np.float32))
            assert np.array_equal(_np(go), (towers > 0).astype(np.float32))
