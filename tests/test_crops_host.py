"""Scan crops (K9), the part that needs no GPU: the numpy oracle against the reference's recorded crops, the case sets, the
lattice helper, and the argument checks of the C entries."""
import ctypes
import os

import numpy as np
import pytest
import torch

import scene_net_amd as sna
from scene_net_amd import _hip

import crops_cases as cc
from scene_net_amd.crops import lattice_boxes


def test_oracle_reproduces_the_reference_crops(golden_dir):
    tile = np.load(os.path.join(golden_dir, "ts40k_sample575_full.npz"))["tile"]
    g = np.load(os.path.join(golden_dir, "scan_crops.npz"))
    xyz = np.ascontiguousarray(tile[:, :3])
    crops = cc.golden_crops(g)
    assert len(crops) == 6 * 3 + 3 + 1
    sizes = []
    for name, row, kind in crops:
        want = np.unpackbits(g[name + "_bits"])[:len(xyz)].astype(bool)
        assert np.array_equal(cc.region_mask(xyz, row, kind), want), name
        sizes.append(int(want.sum()))
    assert min(sizes) >= 0 and max(sizes) > 1000 and len(set(sizes)) > 10, "the crops differ and are not trivial"
    # radius 0 is the z extent (crop_at_locations) and the tower's height (crop_tower_radius)
    assert g["at_radii_used"][0] == xyz[:, 2].max() - xyz[:, 2].min()
    tower = xyz[tile[:, 3] == 15]
    assert g["tower_radii_used"][0] == tower[:, 2].max() - tower[:, 2].min()
    assert np.array_equal(g["tower_baricentre"], np.mean(tower, axis=0))


def test_boundary_claims_hold_in_the_oracle():
    pts, labels, regions, kinds, claims = cc.boundary_case()
    assert len(claims) >= 2 * 18 + 12
    for k, i, member in claims:
        assert bool(cc.region_mask(pts[i:i + 1], regions[k], int(kinds[k]))[0]) is member, (k, i, member)


def test_rim_claims_hold_in_the_oracle():
    pts, labels, regions, kinds, claims = cc.rim_case(1024)
    for k, i, member in claims:
        assert bool(cc.region_mask(pts[i:i + 1], regions[k], int(kinds[k]))[0]) is member, (k, i, member)
    offsets = cc.crop_oracle(pts, labels, regions, kinds)[0]
    sizes = np.diff(offsets).tolist()
    assert sizes[0] == 2 and sizes[1] == 0 and sizes[4] == 2, "at r = 5 the two rim points are the only members; a hair below, none"
    assert sizes[2] == sizes[3] + 1, "at r = 13 the right chunk's rim point is the one member a hair below loses"


def test_contraction_set_is_large_enough():
    pts, labels, regions, kinds, count = cc.contraction_case()
    assert count >= 64 and len(pts) == count == len(regions)
    # the plain sum decides each draw's own disc one way, a contracted sum the other
    from fractions import Fraction
    flipped = 0
    for i in range(count):
        dx, dy = float(pts[i, 0] - cc.CENTRE[0]), float(pts[i, 1] - cc.CENTRE[1])
        r2 = float(regions[i, 2]) ** 2
        plain = dx * dx + dy * dy <= r2
        assert bool(cc.disc_mask(pts[i:i + 1], regions[i, :2], float(regions[i, 2]))[0]) is plain
        fused = [float(Fraction(dx) ** 2 + Fraction(dy * dy)) <= r2, float(Fraction(dy) ** 2 + Fraction(dx * dx)) <= r2]
        flipped += any(f is not plain for f in fused)
    assert flipped == count


def test_nonfinite_case_carries_its_bit_patterns():
    pts, labels, regions, kinds = cc.nonfinite_case()
    b = set(cc.bits(pts).reshape(-1).tolist()) | set(cc.bits(labels).tolist())
    for pattern in (0x7ff8000000001234, 0xfff800000000beef, 0x7ff0000000000077, 0x8000000000000000, 1):
        assert np.array(pattern, dtype=np.uint64).view(np.int64).item() in b, hex(pattern)
    offsets, rows, lab, src = cc.crop_oracle(pts, labels, regions, kinds)
    sizes = np.diff(offsets)
    assert sizes[0] == 0 and sizes[8] == 0 and np.all(sizes[-3:] == 0), "r NaN, min > max and unknown kinds are empty"
    assert sizes[1] > 0 and sizes[3] == sizes[4] > 0, "r = inf admits points; r = -4 behaves as 4"
    assert sizes[11] == 1 and sizes[2] == 1, "a box with min == max and a disc of r = 0 hold the point that sits there"


def test_lattice_regions_cover_the_rectangle():
    with pytest.raises(sna.HipLibraryError, match="no CPU path"):
        sna.lattice_regions((0.0, 0.0), (10.0, 10.0), 5.0, device="cpu")
    r = lattice_boxes((100.0, 200.0), (170.0, 265.0), 30.0, overlap=2.5)
    assert r.shape == (3 * 3, 4)
    assert r[:, 0].min() == 100.0 and r[:, 1].min() == 200.0 and r[:, 2].max() == 170.0 and r[:, 3].max() == 265.0
    xs = sorted(set(map(tuple, r[:, [0, 2]].tolist())))
    assert xs == [(100.0, 132.5), (127.5, 162.5), (157.5, 170.0)], "cells of 30 grown by 2.5, clipped to the rectangle"
    ys = sorted(set(map(tuple, r[:, [1, 3]].tolist())))
    assert ys == [(200.0, 232.5), (227.5, 262.5), (257.5, 265.0)]
    # every point of the rectangle is in a box, and neighbours share 2 * overlap
    rng = np.random.default_rng(5)
    p = np.column_stack([rng.uniform(100, 170, 2000), rng.uniform(200, 265, 2000), np.zeros(2000)])
    p[:4, :2] = [[100, 200], [170, 265], [130, 230], [160, 260]]
    hits = sum(cc.box_mask(p, row).astype(int) for row in r)
    assert hits.min() >= 1 and hits.max() == 4
    with pytest.raises(ValueError):
        lattice_boxes((0, 0), (1, 1), 0.0)


def test_argument_checks_need_no_gpu():
    lib = _hip.load()
    buf = ctypes.create_string_buffer(256)
    p = ctypes.cast(buf, ctypes.c_void_p)
    big = ctypes.c_size_t(1 << 40)
    off = lambda d: ctypes.c_void_p(p.value + d)   # noqa: E731

    def count(pts=p, n=100, regions=p, kinds=p, K=3, ws=p, ws_bytes=big, offsets=p):
        return lib.sn_crop_count(pts, n, regions, kinds, K, ws, ws_bytes, offsets, None)

    def scatter(pts=p, labels=p, n=100, regions=p, kinds=p, K=3, ws=p, ws_bytes=big, offsets=p, capacity=10, out_pts=p,
                out_labels=p, out_src=p):
        return lib.sn_crop_scatter(pts, labels, n, regions, kinds, K, ws, ws_bytes, offsets, capacity, out_pts, out_labels,
                                   out_src, None)

    for call, required in ((count, ("pts", "regions", "ws", "offsets")), (scatter, ("pts", "regions", "ws", "offsets", "out_pts"))):
        for name in required:
            assert call(**{name: None}) == -1, name
            assert b"null" in lib.sn_last_error()
        for n in (0, -5):
            assert call(n=n) == -1
        for K in (0, -1):
            assert call(K=K) == -1
        need = lib.sn_crops_ws_bytes(100, 3)
        assert need == 8 * 3 * 2
        assert call(ws_bytes=ctypes.c_size_t(need - 1)) == -1
        assert b"sn_crops_ws_bytes" in lib.sn_last_error()
        for name in ("pts", "regions", "ws", "offsets"):
            assert call(**{name: off(4)}) == -1, name
            assert b"aligned" in lib.sn_last_error()
        assert call(kinds=off(2)) == -1
        assert call(K=(1 << 16) + 1) == -2 and call(n=(1 << 36) + 1) == -2
        assert b"beyond" in lib.sn_last_error()
    assert scatter(capacity=-1) == -1
    assert b"capacity" in lib.sn_last_error()
    assert scatter(labels=None) == -1 and scatter(out_labels=None) == -1       # one without the other
    assert b"iff" in lib.sn_last_error()
    for name in ("labels", "out_pts", "out_labels", "out_src"):
        assert scatter(**{name: off(4)}) == -1, name


def test_ws_bytes_and_chunk_points():
    lib = _hip.load()
    c = lib.sn_crops_chunk_points()
    assert c == _hip.crops_chunk_points() and c >= 64 and c % 64 == 0
    for n, K in ((0, 1), (-1, 1), (1, 0), (1, -2), ((1 << 36) + 1, 1), (1, (1 << 16) + 1)):
        assert lib.sn_crops_ws_bytes(n, K) == 0, (n, K)
    assert lib.sn_crops_ws_bytes(1 << 33, 4096) > 0, "2^33 points and 4096 regions are served"
    assert lib.sn_crops_ws_bytes(1 << 36, 1 << 16) > 0
    for n, chunks in ((1, 1), (c, 1), (c + 1, 2), (3 * c + 17, 4)):
        assert lib.sn_crops_ws_bytes(n, 5) == 8 * 5 * (chunks + 1)
    with pytest.raises(_hip.HipLibraryError):
        _hip.crops_ws_bytes(0, 1)


def test_cpu_tensors_raise():
    pts, regions = torch.zeros(8, 3, dtype=torch.float64), torch.zeros(1, 4, dtype=torch.float64)
    with pytest.raises(sna.HipLibraryError, match="no CPU path"):
        sna.crop_regions(pts, regions)
    with pytest.raises(sna.HipLibraryError, match="no CPU path"):
        sna.crop_at_locations(pts, torch.zeros(1, 3, dtype=torch.float64), radius=2.0)
    with pytest.raises(sna.HipLibraryError, match="no CPU path"):
        sna.crop_tower_radius(pts, torch.zeros(8), pts[:2], radius=2.0)
    with pytest.raises(sna.HipLibraryError, match="no CPU path"):
        sna.crop_two_towers(pts, torch.zeros(8), pts[:2], pts[2:4])
    with pytest.raises(sna.HipLibraryError, match="no CPU path"):
        sna.crop_tower_samples(pts, torch.zeros(8), [pts[:2]])
    with pytest.raises(sna.HipLibraryError, match="no CPU path"):
        sna.merge_to_scan(torch.zeros(4), torch.zeros(4, dtype=torch.int64), 8)
