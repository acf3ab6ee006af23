"""K17 on the CPU: the Philox restatement against the published known answers, the uniforms, the height thresholds, the two
oracles of tests/thin_cases.py against each other, and the argument checks of every new entry (no GPU is touched)."""
import ctypes

import numpy as np
import pytest

import binning_cases as bc
import thin_cases as tc
from scene_net_amd import _hip
from scene_net_amd.thin import height_thresholds, philox4x32, philox_uniforms, uniform_thresholds


def test_philox_known_answers():
    for counter, key, out in tc.PHILOX_KAT:
        got = philox4x32(np.array(counter, dtype=np.uint64), np.array(key, dtype=np.uint64))
        assert [int(v) for v in got] == list(out), (counter, key)
    # the batched form is the scalar form row by row
    counters = np.array([k[0] for k in tc.PHILOX_KAT], dtype=np.uint64)
    keys = np.array([k[1] for k in tc.PHILOX_KAT], dtype=np.uint64)
    assert np.array_equal(philox4x32(counters, keys), np.array([k[2] for k in tc.PHILOX_KAT], dtype=np.uint32))


def test_uniforms_are_the_53_bit_construction_of_words_0_and_1():
    t = tc.BIG_TILE_ID
    u = philox_uniforms(tc.SEED, t, 1000)
    for j in (0, 5, 999):
        w = philox4x32(np.array([j, 0, t & 0xffffffff, t >> 32], dtype=np.uint64),
                       np.array([tc.SEED & 0xffffffff, tc.SEED >> 32], dtype=np.uint64))
        assert u[j] == ((int(w[0]) >> 5) * 67108864.0 + (int(w[1]) >> 6)) / 9007199254740992.0     # numpy's random_double
    # the tile id and the seed both matter, and a tile's draws do not depend on how many are asked for
    a, b = philox_uniforms(tc.SEED, 3, 1000), philox_uniforms(tc.SEED, 3, 10)
    assert np.array_equal(a[:10], b)
    assert not np.array_equal(a, philox_uniforms(tc.SEED, 4, 1000))
    assert not np.array_equal(a, philox_uniforms(tc.SEED + 1, 3, 1000))
    assert not np.array_equal(a, philox_uniforms(tc.SEED, 3 + 2 ** 32, 1000))


def test_uniforms_range_and_kept_share():
    n, p = 10 ** 6, 0.3
    u = philox_uniforms(tc.SEED, tc.BIG_TILE_ID, n)
    assert u.dtype == np.float64 and u.min() >= 0.0 and u.max() < 1.0
    kept = int((u <= p).sum())
    assert abs(kept - n * p) <= 5.0 * np.sqrt(n * p * (1 - p)), kept


def test_height_thresholds():
    h = height_thresholds(0.8, 64)
    assert h.shape == (64,) and h.dtype == np.float64
    assert h[0] == 0.8 and h[63] == 0.0
    z = 17
    assert h[z] == 0.8 * (1 - z / (64 - 1))      # the reference's expression, operation for operation
    assert np.all(np.diff(h) < 0)
    one = height_thresholds(0.8, 1)
    assert one.shape == (1,) and np.isnan(one).all()
    assert np.array_equal(uniform_thresholds(0.5, 4), np.full(4, 0.5)) and uniform_thresholds(0.25).shape == (1,)


@pytest.mark.parametrize("kind", [tc.Z, tc.VOXEL])
def test_reference_order_against_scan_order(kind):
    dims = (5, 7, 3)
    rng = np.random.default_rng(5)
    thr = rng.random(tc.n_groups(kind, dims))
    # a shuffled cloud with foreign points: the same set, another sequence
    desc, _ = bc.host_desc("own", dims, 1)
    pts = bc.foreign_points(desc[0, :3], desc[0, 3:6], dims, rng, 1500)
    g = tc.groups_of(kind, dims, bc.expected_flat(desc[0], dims, pts))
    assert (g < 0).sum() > 100 and (g >= 0).sum() > 500
    u = rng.random(len(pts))
    ref, scan = tc.reference_order(g, u, thr), tc.scan_order(g, u, thr)
    assert 0.2 * (g >= 0).sum() < len(scan) < 0.8 * (g >= 0).sum()
    assert np.array_equal(np.sort(ref), scan) and not np.array_equal(ref, scan)
    assert not (g[ref] < 0).any()
    # the reference's order: groups by first appearance, scan order inside a group
    first = tc.first_appearance(g, len(thr))
    rank = first[g[ref]]
    assert np.all(np.diff(rank) >= 0) and np.all(np.diff(ref)[np.diff(rank) == 0] > 0)
    # groups visited in ascending first appearance with contiguous members: the two orders are one
    order = np.argsort(np.where(g < 0, g.max() + 1, g), kind="stable")
    gs, us = g[order], u[order]
    assert np.array_equal(tc.reference_order(gs, us, thr), tc.scan_order(gs, us, thr))


def test_threshold_rule_is_literal():
    thr = np.array([0.5, 0.0, np.nan])
    g = np.array([0, 0, 0, 0, 1, 1, 1, 2, 2, -1])
    u = np.array([0.5, np.nextafter(0.5, 1), np.nextafter(0.5, 0), np.nan, 0.0, -0.0, 5e-324, 0.0, np.nan, 0.0])
    assert tc.keep_mask(g, u, thr).tolist() == [True, False, True, False, True, True, False, False, False, False]


def test_argument_checks_need_no_gpu():
    lib = _hip.load()
    buf = ctypes.create_string_buffer(256)
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert p.value % 8 == 0
    off = lambda k: ctypes.c_void_p(p.value + k)   # noqa: E731
    big = ctypes.c_size_t(1 << 20)

    def count(pts=p, offsets=p, total=100, B=2, group=0, desc=None, dims=(4, 4, 4), thr=p, u=p, seed=None, tile_ids=None,
              ws=p, ws_bytes=big, offsets_out=p, unbinned=p, first=None):
        return lib.sn_thin_count(pts, offsets, total, B, group, desc, *dims, thr, u, seed, tile_ids, ws, ws_bytes, offsets_out,
                                 unbinned, first, None)

    def scatter(pts=p, labels=p, offsets=p, total=100, B=2, group=0, desc=None, dims=(4, 4, 4), thr=p, u=p, seed=None,
                tile_ids=None, ws=p, ws_bytes=big, capacity=10, out_pts=p, out_labels=p, out_src=p, out_key=p):
        return lib.sn_thin_scatter(pts, labels, offsets, total, B, group, desc, *dims, thr, u, seed, tile_ids, ws, ws_bytes,
                                   capacity, out_pts, out_labels, out_src, out_key, None)

    for call, required in ((count, ("pts", "offsets", "thr", "ws", "offsets_out", "unbinned")),
                           (scatter, ("pts", "offsets", "thr", "ws", "out_pts"))):
        for name in required:
            kw = {name: None}
            if name == "out_pts":
                kw["capacity"] = 0
            assert call(**kw) == -1, name
            assert b"null" in lib.sn_last_error(), name
        for kw in (dict(total=0), dict(total=-5), dict(B=0), dict(B=-1), dict(group=3), dict(group=-1)):
            assert call(**kw) == -1, kw
        # the uniform: exactly one of u and seed
        assert call(u=p, seed=p) == -1 and b"exactly one" in lib.sn_last_error()
        assert call(u=None, seed=None) == -1 and b"exactly one" in lib.sn_last_error()
        # a grouped rule needs a descriptor and positive extents; without groups neither is looked at
        for group in (1, 2):
            assert call(group=group, desc=None) == -1 and b"descriptor" in lib.sn_last_error()
            assert call(group=group, desc=p, dims=(4, 0, 4)) == -1
            assert call(group=group, desc=p, dims=(4000, 4000, 400)) == -2 and b"LDS" in lib.sn_last_error()
            assert call(group=group, desc=p, dims=(2048, 2048, 512)) == -2 and b"2^31" in lib.sn_last_error()
        assert call(total=(1 << 33) + 1, ws_bytes=ctypes.c_size_t(1 << 40)) == -2
        assert call(B=(1 << 16) + 1) == -2
        need = lib.sn_thin_ws_bytes(100, 2)
        assert call(ws_bytes=ctypes.c_size_t(need - 1)) == -1 and b"sn_thin_ws_bytes" in lib.sn_last_error()
        for name in ("pts", "offsets", "thr", "u", "ws"):
            assert call(**{name: off(4)}) == -1, name
            assert b"aligned" in lib.sn_last_error()
        assert call(u=None, seed=off(4)) == -1 and b"aligned" in lib.sn_last_error()
        assert call(tile_ids=off(4)) == -1 and b"aligned" in lib.sn_last_error()
        assert call(group=1, desc=off(4)) == -1 and b"aligned" in lib.sn_last_error()
    for name in ("offsets_out", "unbinned", "first"):
        assert count(**{name: off(4)}) == -1, name
        assert b"aligned" in lib.sn_last_error()
    assert scatter(capacity=-1) == -1 and b"capacity" in lib.sn_last_error()
    assert scatter(labels=None) == -1 and scatter(out_labels=None) == -1
    for name, k in (("labels", 4), ("out_pts", 4), ("out_labels", 4), ("out_src", 4), ("out_key", 2)):
        assert scatter(**{name: off(k)}) == -1, name
        assert b"aligned" in lib.sn_last_error()


def test_workspace_and_chunk_sizes():
    lib = _hip.load()
    c = lib.sn_thin_chunk_points()
    assert c == _hip.thin_chunk_points() and c >= 64 and c % 64 == 0
    for total, B in ((0, 1), (-1, 1), (1, 0), (1, -2), ((1 << 33) + 1, 1), (1, (1 << 16) + 1)):
        assert lib.sn_thin_ws_bytes(total, B) == 0, (total, B)
    assert lib.sn_thin_ws_bytes(1 << 33, 1 << 16) > 0
    for total, chunks in ((1, 1), (c, 1), (c + 1, 2), (3 * c + 17, 4)):
        # two prefix rows of chunks + 1 words, two bits per row of the batch
        assert lib.sn_thin_ws_bytes(total, 5) == 8 * (2 * (chunks + 1) + 2 * chunks * (c // 64))
    with pytest.raises(_hip.HipLibraryError):
        _hip.thin_ws_bytes(0, 1)
    assert _hip.thin_groups(0, (5, 7, 3)) == 1 and _hip.thin_groups(1, (5, 7, 3)) == 3 and _hip.thin_groups(2, (5, 7, 3)) == 105
