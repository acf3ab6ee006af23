"""Scan merge (K19) without a GPU: every refusal sn_scan_merge documents, through ctypes before any launch; the oracle of
scan_merge_cases against an independent formulation; the host half of kept -> tile_of; no CPU path."""
import ctypes

import numpy as np
import pytest
import torch

import scene_net_amd as sna
from scene_net_amd import _hip
from scene_net_amd.scan_merge import tile_groups, tile_of_kept

import scan_merge_cases as mc

INVALID, UNSUPPORTED = -1, -2


def _call(lib, **kw):
    buf = ctypes.create_string_buffer(256)
    p = ctypes.cast(buf, ctypes.c_void_p).value
    assert p % 16 == 0 or p % 8 == 0
    a = dict(grid=p, dtype=_hip.SN_F32, channels=1, B=4, nx=8, ny=8, nz=8, desc=p, pts=p, n=100, regions=p, kinds=p,
             tile_of=p, K=4, rule=0, fill=0.0, out=p, cover=p)
    a.update(kw)
    rc = lib.sn_scan_merge(a["grid"], a["dtype"], a["channels"], a["B"], a["nx"], a["ny"], a["nz"], a["desc"], a["pts"], a["n"],
                           a["regions"], a["kinds"], a["tile_of"], a["K"], a["rule"], a["fill"], a["out"], a["cover"], None)
    return rc, lib.sn_last_error(), p


def test_refusals_before_any_launch():
    lib = _hip.load()
    for name in ("grid", "desc", "pts", "regions", "out"):
        rc, msg, _ = _call(lib, **{name: None})
        assert rc == INVALID and name.encode() in msg and b"null" in msg, (name, rc, msg)
    for name, word in (("n", b"n must"), ("K", b"K must"), ("B", b"extent"), ("channels", b"extent"), ("nx", b"extent"),
                       ("ny", b"extent"), ("nz", b"extent")):
        for v in (0, -3):
            rc, msg, _ = _call(lib, **{name: v})
            assert rc == INVALID and word in msg, (name, v, rc, msg)
    for rule in (-1, 3):
        rc, msg, _ = _call(lib, rule=rule)
        assert rc == INVALID and b"rule" in msg
    for dtype in (_hip.SN_U8, _hip.SN_BF16, 17):
        rc, msg, _ = _call(lib, dtype=dtype)
        assert rc == INVALID and b"dtype" in msg
    rc, msg, _ = _call(lib, tile_of=None, B=3, K=4)
    assert rc == INVALID and b"tile_of" in msg
    _, _, p = _call(lib, rule=9)
    for name, off in (("pts", 4), ("regions", 4), ("desc", 4), ("kinds", 2), ("tile_of", 2), ("cover", 2), ("grid", 2),
                      ("out", 2)):
        rc, msg, _ = _call(lib, **{name: p + off})
        assert rc == INVALID and b"aligned" in msg, (name, rc, msg)
    for name in ("grid", "out"):       # element size: 4 bytes serve f32, not f64
        rc, msg, _ = _call(lib, dtype=_hip.SN_F64, **{name: p + 4})
        assert rc == INVALID and b"aligned" in msg
    rc, msg, _ = _call(lib, n=(1 << 36) + 1)
    assert rc == UNSUPPORTED and b"2^36" in msg
    rc, msg, _ = _call(lib, K=65537, B=65537)
    assert rc == UNSUPPORTED and b"65536" in msg
    rc, msg, _ = _call(lib, channels=65536)
    assert rc == UNSUPPORTED and b"channels" in msg
    rc, msg, _ = _call(lib, nx=4000, ny=4000, nz=190)      # 8193 edges: 8 bytes above 64 KiB
    assert rc == UNSUPPORTED and b"64 KiB" in msg
    assert (_hip.SN_MERGE_MAX, _hip.SN_MERGE_MEAN, _hip.SN_MERGE_INTERIOR) == (0, 1, 2)


def test_the_inputs_hold_what_they_are_there_for():
    counts = mc.check_inputs()
    assert len(counts) == 5


@pytest.mark.parametrize("kind", ["own", "foreign", "sized"])
def test_oracle_max_equals_a_scatter_formulation(kind):
    pts, regions, kinds, _ = mc.main_scan()
    dims = mc.CAPACITY if kind == "sized" else mc.DIMS[0]
    desc, own = mc.main_desc(dims, kind)
    grid = mc.random_grid(10, 3, dims, np.float32, 5)
    idx = mc.repeated_regions(65)
    for reg, kin, tile_of in ((regions, kinds, None), (regions[idx], kinds[idx], idx)):
        got, cover = mc.merge_oracle(grid, desc, dims, pts, reg, kin, tile_of, mc.MAX, -7.0, own)
        want = mc.max_by_scatter(grid, desc, dims, pts, reg, kin, tile_of, -7.0, own)
        assert mc.same_bits(got, want)
        assert np.array_equal(cover == 0, (got == -7.0).all(axis=0))


def test_oracle_rules_on_the_tie_points():
    pts, regions, kinds, ties = mc.main_scan()
    desc, _ = mc.main_desc(mc.DIMS[1])
    grid = mc.random_grid(10, 1, mc.DIMS[1], np.float64, 6)
    out, cover = mc.merge_oracle(grid, desc, mc.DIMS[1], pts, regions, kinds, None, mc.INTERIOR, 0.0)
    g = grid.reshape(10, -1)
    import binning_cases as bc
    for i in ties:
        f = bc.expected_flat(desc[mc.TIE_WINNER], mc.DIMS[1], pts[i:i + 1])[0]
        assert out[0, i] == g[mc.TIE_WINNER, f]
    mean, _ = mc.merge_oracle(grid, desc, mc.DIMS[1], pts, regions, kinds, None, mc.MEAN, 0.0)
    i = ties[2]
    vals = [g[t, bc.expected_flat(desc[t], mc.DIMS[1], pts[i:i + 1])[0]] for t in (0, 1, 3, 4)]
    assert mean[0, i] == (((vals[0] + vals[1]) + vals[2]) + vals[3]) / 4.0


def test_kept_to_tile_of():
    assert tile_of_kept([0, 2, 3], 5).tolist() == [0, -1, 1, 2, -1]
    assert tile_of_kept([3, 0], 4).tolist() == [1, -1, -1, 0] and tile_of_kept([], 2).tolist() == [-1, -1]
    assert tile_of_kept([0, 1], 2).dtype == np.int32
    for bad in ([0, 5], [-1], [1, 1]):
        with pytest.raises(ValueError):
            tile_of_kept(bad, 5)
    assert [list(r) for r in tile_groups(5, 2)] == [[0, 1], [2, 3], [4]] and [list(r) for r in tile_groups(3, 32)] == [[0, 1, 2]]
    with pytest.raises(ValueError):
        tile_groups(3, 0)


def test_cpu_tensors_are_refused():
    pts, regions, kinds, _ = mc.main_scan()
    desc, _ = mc.main_desc(mc.DIMS[1])
    t = torch.from_numpy
    with pytest.raises(sna.HipLibraryError, match="no CPU path"):
        sna.scan_predictions(t(mc.random_grid(10, 1, mc.DIMS[1], np.float32, 1)), t(pts), t(regions), t(kinds), t(desc))
    model = sna.SceneNet({"cy": 1}, (3, 3, 3))
    with pytest.raises(sna.HipLibraryError, match="no CPU path"):
        sna.segment_scan(model, t(pts))
    with pytest.raises(sna.HipLibraryError, match="no CPU path"):
        sna.classify_las("in.las", "out.las", model, 0.5)
    with pytest.raises(ValueError, match="rule"):
        sna.scan_predictions(t(mc.random_grid(10, 1, mc.DIMS[1], np.float32, 1)), t(pts), t(regions), t(kinds), t(desc), rule="min")
