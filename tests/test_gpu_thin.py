"""K17 on the GPU: sn_thin_count / sn_thin_scatter and the layers above them against the oracles of tests/thin_cases.py.
Every comparison is exact: integers as they are, fp64 as int64 views.  Seams of the 1024-row chunk, batches with an odd
start offset, a one-point and an empty tile, buffers offset by one element, the inclusive threshold and the NaN rule,
K1's binning of foreign points, the built-in generator against its numpy restatement, the reference's row order, capture."""
import numpy as np
import pytest
import torch

import binning_cases as bc
import thin_cases as tc
import scene_net_amd as sna
from scene_net_amd import _hip

pytestmark = pytest.mark.gpu

GUARD = 5                      # sentinel rows behind every output
SENT_F = -7.25e300             # what an untouched fp64 row holds
SENT_I = -99


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


def shifted(arr, dev, shift):
    """The array on the device, `shift` elements into a larger buffer (8-byte aligned, not 16)."""
    flat = torch.from_numpy(np.ascontiguousarray(arr)).reshape(-1)
    buf = torch.empty(flat.numel() + shift, dtype=flat.dtype, device=dev)
    view = buf[shift:]
    view.copy_(flat)
    return view.reshape(arr.shape)


def run(dev, tiles, labels, kind, dims, desc, thr, us=None, seed=None, tile_ids=None, want_src=True, want_key=True,
        want_first=True, capacity=None, shift=0):
    """One count + scatter through the ctypes layer with sentinel-filled outputs; returns numpy copies of everything."""
    sizes = [len(t) for t in tiles]
    total, B = int(sum(sizes)), len(tiles)
    G = tc.n_groups(kind, dims)
    pts = shifted(np.concatenate(tiles).astype(np.float64), dev, shift)
    lab = None if labels is None else shifted(np.concatenate(labels).astype(np.float64), dev, shift)
    offsets = shifted(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64), dev, shift)
    d = None if kind == tc.NONE else shifted(np.asarray(desc, dtype=np.float64), dev, shift)
    t = shifted(np.asarray(thr, dtype=np.float64).reshape(B, G), dev, shift)
    u = None if us is None else shifted(np.concatenate(us).astype(np.float64), dev, shift)
    s = None
    if seed is not None:
        s = shifted(np.array([seed], dtype=np.uint64).view(np.int64), dev, shift)
    ids = None if tile_ids is None else shifted(np.asarray(tile_ids, dtype=np.uint64).view(np.int64), dev, shift)
    ws = torch.empty(_hip.thin_ws_bytes(total, B) // 8 + shift, dtype=torch.int64, device=dev)[shift:]
    offsets_out = torch.full((B + 1 + shift,), SENT_I, dtype=torch.int64, device=dev)[shift:]
    unbinned = torch.full((B + shift,), SENT_I, dtype=torch.int64, device=dev)[shift:]
    first = torch.full((B * G + shift,), 12345, dtype=torch.int64, device=dev)[shift:].reshape(B, G) if want_first else None
    rule = (offsets, kind, d, dims, t, u, s, ids, ws)
    _hip.thin_count(pts, *rule, offsets_out, unbinned, first)
    off = offsets_out.cpu().numpy()
    kept = int(off[-1])
    cap = kept if capacity is None else int(capacity)
    rows = cap + GUARD
    out_pts = torch.full((rows * 3 + shift,), SENT_F, dtype=torch.float64, device=dev)[shift:].reshape(rows, 3)
    out_lab = None if lab is None else torch.full((rows + shift,), SENT_F, dtype=torch.float64, device=dev)[shift:]
    out_src = torch.full((rows + shift,), SENT_I, dtype=torch.int64, device=dev)[shift:] if want_src else None
    # (an int32 buffer: one element of shift is 4 bytes, the alignment the entry asks of out_key)
    out_key = torch.full((rows + shift,), SENT_I, dtype=torch.int32, device=dev)[shift:] if want_key else None
    if cap > 0:
        _hip.thin_scatter(pts, lab, *rule, out_pts, out_lab, out_src, out_key, capacity=cap)
    torch.cuda.synchronize()
    get = lambda x: None if x is None else x.cpu().numpy()   # noqa: E731
    return dict(offsets=off, unbinned=get(unbinned), first=get(first), pts=get(out_pts), labels=get(out_lab),
                src=get(out_src), key=get(out_key), kept=kept, cap=cap)


def check(out, exp, tiles, labels, kind):
    """Everything one run returns against the expectation of thin_cases.expected_batch."""
    packed = np.concatenate(tiles).astype(np.float64)
    assert np.array_equal(out["offsets"], exp["offsets"])
    assert np.array_equal(out["unbinned"], exp["unbinned"])
    if out["first"] is not None:
        assert np.array_equal(out["first"], exp["first"])
    n = min(out["kept"], out["cap"])
    src = exp["src"][:n]
    assert np.array_equal(bits(out["pts"][:n]), bits(packed[src]))
    assert np.all(out["pts"][n:] == SENT_F), "rows beyond the result or the capacity were touched"
    if labels is not None:
        assert np.array_equal(bits(out["labels"][:n]), bits(np.concatenate(labels)[src]))
        assert np.all(out["labels"][n:] == SENT_F)
    if out["src"] is not None:
        assert np.array_equal(out["src"][:n], src) and np.all(out["src"][n:] == SENT_I)
    if out["key"] is not None:
        assert np.array_equal(out["key"][:n], exp["key"][:n]) and np.all(out["key"][n:] == SENT_I)


# ---------------------------------------------------------------- seams
def seam_totals():
    c = _hip.thin_chunk_points()
    return [1, 63, 64, 65, 255, 257, c - 1, c, c + 1, 3 * c + 17]


@pytest.mark.parametrize("idx", range(10))
def test_seams_one_tile(hip_device, idx):
    total = seam_totals()[idx]
    rng = np.random.default_rng(100 + idx)
    tile = bc.UTM + rng.random((total, 3)) * 30.0
    tile[rng.random(total) < 0.02] = np.nan          # without groups a NaN row is a row like any other
    lab = bc.LABELS[rng.integers(0, 4, total)]
    thr = np.array([[0.5]])
    u = tc.philox_uniforms(tc.SEED + idx, 0, total)
    exp = tc.expected_batch([tile], tc.NONE, (1, 1, 1), None, thr, [u])
    if total >= 255:
        assert 0.3 * total < len(exp["src"]) < 0.7 * total      # not vacuous: the oracle itself
    for shift, with_all in ((0, True), (1, False), (1, True)):
        out = run(hip_device, [tile], [lab] if with_all else None, tc.NONE, (1, 1, 1), None, thr, seed=tc.SEED + idx,
                  want_src=with_all, want_key=with_all, want_first=with_all, shift=shift)
        check(out, exp, [tile], [lab] if with_all else None, tc.NONE)
        if total >= 255:
            assert 0.3 * total < out["kept"] < 0.7 * total
    # explicit uniforms give the same rows; a capacity below the result leaves the rest alone
    out = run(hip_device, [tile], [lab], tc.NONE, (1, 1, 1), None, thr, us=[u], capacity=len(exp["src"]) // 2)
    check(out, exp, [tile], [lab], tc.NONE)


def test_prefix_carries_into_the_second_scan_tile(hip_device):
    """The prefix kernel scans kept / lost in tiles of 256 threads x 8 slots = 2048 chunks and carries the running total
    from one tile to the next.  One chunk more than a tile, and a tile of the batch that starts inside that chunk: its
    offsets_out is bits_before on a prefix that holds the carry."""
    c = _hip.thin_chunk_points()
    tile = 256 * 8                                   # kScanThreads * kScanItems of scan.h
    total = (tile + 1) * c + 5
    cuts = [0, 1000, tile * c + 100, total]
    rng = np.random.default_rng(2049)
    packed = bc.UTM + rng.random((total, 3)) * 30.0
    tiles = [packed[a:b] for a, b in zip(cuts[:-1], cuts[1:])]
    u = rng.random(total)
    us = [u[a:b] for a, b in zip(cuts[:-1], cuts[1:])]
    thr = np.array([[0.45], [0.5], [0.55]])
    exp = tc.expected_batch(tiles, tc.NONE, (1, 1, 1), None, thr, us)
    src = exp["src"]
    assert (src < tile * c).sum() > 0.4 * tile * c and (src >= tile * c + 100).sum() > 300    # kept rows on both sides
    assert 20 < ((src >= tile * c) & (src < tile * c + 100)).sum() < 100            # ... and between the two seams
    out = run(hip_device, tiles, None, tc.NONE, (1, 1, 1), None, thr, us=us)
    check(out, exp, tiles, None, tc.NONE)
    assert out["offsets"][2] > 0.4 * tile * c and out["kept"] - out["offsets"][2] > 300


@pytest.mark.parametrize("kind", [tc.Z, tc.VOXEL])
def test_seams_grouped(hip_device, kind):
    c = _hip.thin_chunk_points()
    dims = (5, 7, 3)
    for total in (1, 65, c - 1, c + 1, 3 * c + 17):
        tile = tc.cube_cloud(total, 7 + total)
        desc = tc.own_desc(tile, dims)[None]
        thr = np.full((1, tc.n_groups(kind, dims)), 0.5)
        u = tc.philox_uniforms(11, 0, total)
        exp = tc.expected_batch([tile], kind, dims, desc, thr, [u])
        if total >= 255:
            assert 0.3 * total < len(exp["src"]) < 0.7 * total
        for want_key in (False, True):          # the scatter reads the count's bits, or decides again to find the groups
            out = run(hip_device, [tile], None, kind, dims, desc, thr, seed=11, shift=1, want_key=want_key)
            check(out, exp, [tile], None, kind)


# ---------------------------------------------------------------- batches, binning, generator
def foreign_case(dims, with_empty):
    desc, _ = bc.host_desc("own", dims, 3)
    tiles, labels = bc.foreign_batch(desc, dims)
    if with_empty:
        tiles = [tiles[0], np.empty((0, 3)), tiles[1], tiles[2]]
        labels = [labels[0], np.empty((0,)), labels[1], labels[2]]
        desc = desc[[0, 1, 1, 2]]
    return desc, tiles, labels


@pytest.mark.parametrize("dims", [(5, 7, 3), (64, 64, 64)])
@pytest.mark.parametrize("kind", [tc.Z, tc.VOXEL])
@pytest.mark.parametrize("with_empty", [False, True])
def test_foreign_batch_binning_and_generator(hip_device, dims, kind, with_empty):
    desc, tiles, labels = foreign_case(dims, with_empty)
    B, G = len(tiles), tc.n_groups(kind, dims)
    assert len(tiles[0]) == 1001 and len(tiles[-2]) == 1           # an odd start offset, a one-point tile
    ids = [tc.BIG_TILE_ID + 3 * b for b in range(B)]
    rng = np.random.default_rng(3)
    thr = 0.4 + 0.2 * rng.random((B, G))                   # around 0.5, another one per tile and group
    us = [tc.philox_uniforms(tc.SEED, ids[b], len(t)) for b, t in enumerate(tiles)]
    exp = tc.expected_batch(tiles, kind, dims, desc, thr, us)
    binned = sum(int((g >= 0).sum()) for g in exp["groups"])
    assert exp["unbinned"].sum() > 100 and exp["unbinned"][-2] == 1      # the one-point tile's point is outside
    assert 0.3 * binned < len(exp["src"]) < 0.7 * binned
    for shift in (0, 1):
        out = run(hip_device, tiles, labels, kind, dims, desc, thr, seed=tc.SEED, tile_ids=ids, shift=shift)
        check(out, exp, tiles, labels, kind)
        assert 0.3 * binned < out["kept"] < 0.7 * binned
    # unbinned rows never come out
    packed_groups = np.concatenate(exp["groups"])
    assert (packed_groups[out["src"][:out["kept"]]] >= 0).all()
    # no first, no key, no src, no labels: the plain bitmask scatter
    out = run(hip_device, tiles, None, kind, dims, desc, thr, seed=tc.SEED, tile_ids=ids, want_src=False, want_key=False,
              want_first=False)
    check(out, exp, tiles, None, kind)


def test_tile_is_thinned_alike_wherever_it_sits(hip_device):
    dims = (5, 7, 3)
    c = _hip.thin_chunk_points()
    mine = tc.cube_cloud(2 * c + 300, 21)                  # j runs across two chunk seams
    others = [tc.cube_cloud(777, 22), tc.cube_cloud(1500, 23)]
    thr_row = np.full(3, 0.5)

    def rows_of(tiles, ids, seed):
        desc = np.stack([tc.own_desc(t, dims) for t in tiles])
        thr = np.tile(thr_row, (len(tiles), 1))
        us = [tc.philox_uniforms(seed, ids[b], len(t)) for b, t in enumerate(tiles)]
        exp = tc.expected_batch(tiles, tc.Z, dims, desc, thr, us)
        out = run(hip_device, tiles, None, tc.Z, dims, desc, thr, seed=seed, tile_ids=ids)
        check(out, exp, tiles, None, tc.Z)
        b = ids.index(5)
        start = sum(len(t) for t in tiles[:b])
        return out["src"][out["offsets"][b]:out["offsets"][b + 1]] - start

    first = rows_of([mine] + others, [5, 6, 7], tc.SEED)
    last = rows_of([others[1], others[0], mine], [9, 2 ** 40, 5], tc.SEED)
    assert 0.3 * len(mine) < len(first) < 0.7 * len(mine)
    assert np.array_equal(first, last)
    assert np.array_equal(first, rows_of([mine] + others, [5, 6, 7], tc.SEED))        # same seed: identical
    assert not np.array_equal(first, rows_of([mine] + others, [5, 6, 7], tc.SEED + 1))
    assert np.array_equal(first, rows_of([others[0], mine], [5 + 2 ** 32, 5], tc.SEED))       # second of two, after a look-alike id
    # without tile_ids the id is the tile's index in the batch
    tiles = [others[0], mine]
    desc = np.stack([tc.own_desc(t, dims) for t in tiles])
    thr = np.tile(thr_row, (2, 1))
    exp = tc.expected_batch(tiles, tc.Z, dims, desc, thr, [tc.philox_uniforms(3, b, len(t)) for b, t in enumerate(tiles)])
    check(run(hip_device, tiles, None, tc.Z, dims, desc, thr, seed=3), exp, tiles, None, tc.Z)


# ---------------------------------------------------------------- the threshold's edge
@pytest.mark.parametrize("dims", [(5, 7, 3), (64, 64, 64)])
def test_threshold_edge(hip_device, dims):
    n = 6000
    tile = tc.cube_cloud(n, 31)
    desc = tc.own_desc(tile, dims)[None]
    g = tc.groups_of(tc.Z, dims, bc.expected_flat(desc[0], dims, tile))
    nz = dims[2]
    thr = sna.height_thresholds(0.8, nz)
    assert thr[0] == 0.8 and thr[-1] == 0.0
    rng = np.random.default_rng(32)
    u = rng.random(n)
    for z in range(nz):
        members = np.flatnonzero(g == z)
        assert len(members) >= 7, "every slab must hold the seven probes"
        t = thr[z]
        u[members[:7]] = [t, np.nextafter(t, np.inf), np.nextafter(t, -np.inf), 0.0, -0.0, np.nan, 1.0]
    for thr_row in (thr, np.where(np.arange(nz) == 1, np.nan, thr)):          # and a NaN on the threshold's side
        exp = tc.expected_batch([tile], tc.Z, dims, desc, thr_row[None], [u])
        kept = set(exp["src"].tolist())
        for z in range(nz):
            m = np.flatnonzero(g == z)[:7]
            if np.isnan(thr_row[z]):
                assert not kept & set(m.tolist())
                continue
            assert m[0] in kept and m[1] not in kept and m[5] not in kept          # inclusive, one ulp above, NaN
            assert (m[3] in kept) and (m[4] in kept)                               # 0.0 and -0.0 <= every threshold, 0 too
            assert m[2] in kept                                                    # one ulp below (below 0: the negative denormal)
            assert m[6] not in kept
        out = run(hip_device, [tile], None, tc.Z, dims, desc, thr_row[None], us=[u])
        check(out, exp, [tile], None, tc.Z)


# ---------------------------------------------------------------- the layers above
def test_thin_points_scan_order_keep_all_and_none(hip_device):
    rng = np.random.default_rng(41)
    tiles = [bc.UTM + rng.random((n, 3)) * 10.0 for n in (1300, 1, 700)]
    tiles[0][5] = [np.nan, -0.0, np.inf]
    labels = [bc.LABELS[rng.integers(0, 4, len(t))] for t in tiles]
    batch = sna.PointBatch.from_tiles(tiles, labels, device=hip_device)
    packed, lab = np.concatenate(tiles), np.concatenate(labels)
    everything = sna.thin_points(batch, keep=1.0, seed=5)
    assert everything.batch.sizes == batch.sizes and everything.key is None and everything.first is None
    assert np.array_equal(bits(everything.batch.pts.cpu().numpy()), bits(packed))
    assert np.array_equal(bits(everything.batch.labels.cpu().numpy()), bits(lab))
    assert np.array_equal(everything.src.cpu().numpy(), np.arange(len(packed)))
    assert np.array_equal(everything.batch.offsets.cpu().numpy(), batch.offsets.cpu().numpy())
    nothing = sna.thin_points(batch, keep=0.0, seed=5)
    zero = np.concatenate([np.flatnonzero(tc.philox_uniforms(5, b, len(t)) <= 0.0) + sum(map(len, tiles[:b]))
                           for b, t in enumerate(tiles)])                      # a draw of exactly 0: the oracle decides
    assert np.array_equal(nothing.src.cpu().numpy(), zero) and nothing.batch.pts.shape == (len(zero), 3)
    half = sna.thin_points(batch, keep=0.5, seed=5, want_key=True)
    want = np.concatenate([np.flatnonzero(tc.philox_uniforms(5, b, len(t)) <= 0.5) + sum(map(len, tiles[:b]))
                           for b, t in enumerate(tiles)])
    assert 0.3 * len(packed) < len(want) < 0.7 * len(packed)
    assert np.array_equal(half.src.cpu().numpy(), want) and not half.key.any()
    assert np.array_equal(bits(half.batch.pts.cpu().numpy()), bits(packed[want]))
    assert sum(half.batch.sizes) == len(want) and half.unbinned.cpu().tolist() == [0, 0, 0]
    # CPU tensors raise: there is no CPU path
    with pytest.raises(sna.HipLibraryError):
        sna.thin_points(torch.zeros((4, 3), dtype=torch.float64), keep=0.5, seed=1)


def test_thin_points_with_a_capacity_a_given_grid_and_thresholds_per_tile(hip_device):
    dims = (8, 8, 4)
    tiles = [tc.cube_cloud(1500, 45), tc.cube_cloud(600, 46)]
    batch = sna.PointBatch.from_tiles(tiles, device=hip_device)
    desc, _ = _hip.voxel_prepare(batch.pts, batch.offsets, dims, regular=True)
    rng = np.random.default_rng(47)
    thr = 0.4 + 0.2 * rng.random((2, 4))
    us = [rng.random(len(t)) for t in tiles]
    exp = tc.expected_batch(tiles, tc.Z, dims, desc.cpu().numpy(), thr, us)
    kept = int(exp["offsets"][-1])
    assert 0.3 * 2100 < kept < 0.7 * 2100
    out = sna.thin_points(batch, thresholds=torch.from_numpy(thr).to(hip_device), group="z", grids=desc, voxelgrid_dims=dims,
                          u=np.concatenate(us), want_key=True, capacity=2100)
    assert out.batch.pts.shape == (2100, 3) and out.batch.sizes == batch.sizes      # the input's sizes: upper bounds
    assert np.array_equal(out.batch.offsets.cpu().numpy(), exp["offsets"])
    assert np.array_equal(out.src.cpu().numpy()[:kept], exp["src"]) and np.array_equal(out.key.cpu().numpy()[:kept], exp["key"])
    assert np.array_equal(bits(out.batch.pts.cpu().numpy()[:kept]), bits(np.concatenate(tiles)[exp["src"]]))
    with pytest.raises(ValueError):
        sna.thin_points(batch, keep=0.5, seed=1, group="z", order="reference", capacity=10)


def test_height_rule_on_one_slab_keeps_nothing(hip_device):
    tile = tc.cube_cloud(500, 51)
    out = sna.thin_points(torch.from_numpy(tile).to(hip_device), keep=0.8, rule="height", voxelgrid_dims=(4, 4, 1), seed=1)
    assert out.batch.pts.shape == (0, 3) and out.batch.sizes == (0,) and out.unbinned.cpu().tolist() == [0]


@pytest.mark.parametrize("which", ["downsampling", "downsampling_relative_height"])
def test_mirrors_give_the_reference_order(hip_device, which):
    n, dims, seed = 4000, (64, 64, 64), 77
    xyz = tc.cube_cloud(n, 61)                               # shuffled: voxels and slabs appear in no order
    classes = np.random.default_rng(62).integers(0, 20, n)
    d_xyz = torch.from_numpy(xyz).to(hip_device)
    desc, _ = _hip.voxel_prepare(d_xyz, torch.tensor([0, n], device=hip_device), dims, regular=True)
    host = tc.own_desc(xyz, dims)
    assert np.array_equal(bits(desc.cpu().numpy()[0]), bits(host))        # the grid both sides bin with
    flat = bc.expected_flat(host, dims, xyz)
    u = tc.philox_uniforms(seed, 0, n)
    if which == "downsampling":
        p, g = 0.5, tc.groups_of(tc.VOXEL, dims, flat)
        order = tc.reference_order(g, u, sna.uniform_thresholds(p, 64 ** 3))
        got_xyz, got_cls = sna.downsampling(d_xyz, torch.from_numpy(classes).to(hip_device), p, seed=seed)
    else:
        p, g = 0.8, tc.groups_of(tc.Z, dims, flat)
        order = tc.reference_order(g, u, sna.height_thresholds(p, 64))
        got_xyz, got_cls = sna.downsampling_relative_height(d_xyz, torch.from_numpy(classes).to(hip_device), p, seed=seed)
    assert 0.3 * n < len(order) < 0.7 * n
    assert not np.array_equal(order, np.sort(order))                      # the reference's order is not scan order here
    assert got_cls.dtype == torch.int64
    assert np.array_equal(bits(got_xyz.cpu().numpy()), bits(xyz[order]))
    assert np.array_equal(got_cls.cpu().numpy(), classes[order])
    # arrays in, arrays out, explicit uniforms: the same rows
    fn = getattr(sna, which)
    np_xyz, np_cls = fn(xyz, classes.astype(np.int32), p, u=u)
    assert isinstance(np_xyz, np.ndarray) and np_cls.dtype == np.int32
    assert np.array_equal(bits(np_xyz), bits(xyz[order])) and np.array_equal(np_cls, classes[order])


def test_thin_points_callable_advances_its_seed(hip_device):
    tile = tc.cube_cloud(3000, 71)
    batch = sna.PointBatch.from_tiles([tile], device=hip_device)
    batch.tile_ids = torch.tensor([tc.BIG_TILE_ID], dtype=torch.int64, device=hip_device)
    thin = sna.ThinPoints(0.5, "uniform", seed=9)
    for step in range(2):
        out = thin(batch)
        want = np.flatnonzero(tc.philox_uniforms(9 + step, tc.BIG_TILE_ID, len(tile)) <= 0.5)
        assert np.array_equal(thin.last.src.cpu().numpy(), want) and out.sizes == (len(want),)
        assert out.tile_ids is batch.tile_ids
    thin.reseed(9)
    thin(batch)
    assert np.array_equal(thin.last.src.cpu().numpy(), np.flatnonzero(tc.philox_uniforms(9, tc.BIG_TILE_ID, len(tile)) <= 0.5))


# ---------------------------------------------------------------- capture
def test_captured_count_and_scatter_follow_the_seed_tensor(hip_device):
    dev, dims = hip_device, (5, 7, 3)
    tiles = [tc.cube_cloud(1500, 81), tc.cube_cloud(900, 82)]
    total, B, G = 2400, 2, 3
    desc_h = np.stack([tc.own_desc(t, dims) for t in tiles])
    thr_h = np.tile(sna.height_thresholds(0.9, 3), (2, 1))
    pts = torch.from_numpy(np.concatenate(tiles)).to(dev)
    offsets = torch.tensor([0, 1500, 2400], dtype=torch.int64, device=dev)
    desc, thr = torch.from_numpy(desc_h).to(dev), torch.from_numpy(thr_h).to(dev)
    seed = torch.zeros(1, dtype=torch.int64, device=dev)
    ws = torch.empty(_hip.thin_ws_bytes(total, B) // 8, dtype=torch.int64, device=dev)
    offsets_out = torch.empty(B + 1, dtype=torch.int64, device=dev)
    unbinned = torch.empty(B, dtype=torch.int64, device=dev)
    first = torch.empty((B, G), dtype=torch.int64, device=dev)
    out_pts = torch.empty((total, 3), dtype=torch.float64, device=dev)
    out_src = torch.empty(total, dtype=torch.int64, device=dev)
    out_key = torch.empty(total, dtype=torch.int32, device=dev)
    rule = (offsets, tc.Z, desc, dims, thr, None, seed, None, ws)

    def launch():
        _hip.thin_count(pts, *rule, offsets_out, unbinned, first)
        _hip.thin_scatter(pts, None, *rule, out_pts, None, out_src, out_key)

    def snapshot():
        torch.cuda.synchronize()
        return [t.cpu().numpy().copy() for t in (offsets_out, unbinned, first, out_pts, out_src, out_key)]

    launch()                                                     # (eager first: the kernels are loaded)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch()
    for s in (tc.SEED, 4, tc.SEED):
        seed.fill_(np.array([s], dtype=np.uint64).view(np.int64)[0])
        for t in (out_pts, out_src, out_key):
            t.fill_(0)
        graph.replay()
        replayed = snapshot()
        for t in (out_pts, out_src, out_key):
            t.fill_(0)
        launch()
        eager = snapshot()
        for a, b in zip(replayed, eager):
            assert np.array_equal(a.view(np.int64) if a.dtype == np.float64 else a, b.view(np.int64) if b.dtype == np.float64 else b)
        exp = tc.expected_batch(tiles, tc.Z, dims, desc_h, thr_h, [tc.philox_uniforms(s, b, len(t)) for b, t in enumerate(tiles)])
        assert np.array_equal(replayed[0], exp["offsets"]) and np.array_equal(replayed[4][:exp["offsets"][-1]], exp["src"])
        assert 0.25 * total < exp["offsets"][-1] < 0.7 * total
