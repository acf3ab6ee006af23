"""Voxel clouds (K16), the part that needs no GPU: the numpy restatement against the reference's recorded rows, the colour
table, the argument checks of the C entries and the errors of the Python layer."""
import ctypes
import os

import numpy as np
import pytest
import torch

import scene_net_amd as sna
from scene_net_amd import _hip

import voxel_cloud_cases as vc


def _golden(golden_dir):
    return np.load(os.path.join(golden_dir, "voxel_cloud.npz"))


def test_restatement_equals_the_reference_rows(golden_dir):
    g = _golden(golden_dir)
    names = [str(n) for n in g["names"]]
    assert len(names) >= 12
    seen_none = seen_empty = 0
    for name, mode, r in zip(names, g["modes"], g["rs"]):
        grid, want = g[name + "_grid"], g[name + "_rows"]
        table = g[f"jet_{int(r)}"] if str(mode) == "ranges" else None
        got = vc.restate(grid, str(mode), int(r), table)
        if g[name + "_none"][0]:
            assert got is None, name
            seen_none += 1
            continue
        assert got is not None and got.dtype == np.float64 and got.shape == want.shape, name
        assert got.tobytes() == want.tobytes(), name
        seen_empty += want.shape == (0, 6)
    assert seen_none >= 2 and seen_empty >= 2, "an all-zero and an all-filtered grid are among the cases"


def test_golden_grids_are_the_case_set_and_sit_on_the_seams(golden_dir):
    g = _golden(golden_dir)
    cases = vc.golden_cases()
    assert [c[0] for c in cases] == [str(n) for n in g["names"]]
    for name, grid, mode, r in cases:
        assert grid.tobytes() == g[name + "_grid"].tobytes() and grid.dtype == g[name + "_grid"].dtype, name
        assert max(grid.shape) <= 9 and grid.size <= 9 * 8 * 7
    for r in (2, 5, 10, 17):
        lin, step = vc.lin_step(r)
        grid = g[f"ranges_r{r}_f64_grid"]
        flat = grid.reshape(-1)
        assert lin[1] in flat and np.nextafter(lin[1], 2.0) in flat and 1.0 in flat
        assert (flat < 0).any() and (flat > 1).any() and np.signbit(flat[flat == 0]).any(), "negatives, above 1, a -0.0"
        # neighbours one ulp apart that take different table rows: the bin boundaries are hit
        rows = np.argmin(np.abs(flat[:, None] - lin - step), axis=-1)
        order = np.argsort(flat)
        close = np.diff(flat[order]) <= 4 * np.spacing(np.abs(flat[order][1:]))
        assert (close & (np.diff(rows[order]) != 0)).sum() >= min(r, 3) - 1, r


def test_jet_ranges():
    t = sna.jet_ranges(10)
    assert t.shape == (10, 3) and t.dtype == np.float64 and np.all(t[0] == 1.0)
    cm = pytest.importorskip("matplotlib.cm")
    for r in (10, 2, 17):
        want = np.array(cm.jet(np.linspace(0, 1, r)))[:, :3]
        want[0] = 1.0
        assert sna.jet_ranges(r).tobytes() == want.astype(np.float64).tobytes(), r
    for r in (1, 33, 0):
        with pytest.raises(ValueError):
            sna.jet_ranges(r)


def test_jet_ranges_agrees_with_the_recorded_tables(golden_dir):
    g = _golden(golden_dir)
    assert sna.jet_ranges(10).tobytes() == g["jet_10"].tobytes()


def test_argument_checks_need_no_gpu():
    lib = _hip.load()
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) // 16 * 16)   # (every call below is refused before any launch)
    big = ctypes.c_size_t(1 << 40)
    off = lambda d: ctypes.c_void_p(p.value + d)   # noqa: E731
    D, R = _hip.SN_CLOUD_DENSITY, _hip.SN_CLOUD_RANGES

    def count(grid=p, dtype=_hip.SN_F64, B=2, n0=4, n1=5, n2=6, mode=R, r=10, desc=None, ws=p, ws_bytes=big, offsets=p,
              bad=p):
        return lib.sn_voxel_cloud_count(grid, dtype, B, n0, n1, n2, mode, r, desc, ws, ws_bytes, offsets, bad, None)

    def scatter(grid=p, dtype=_hip.SN_F64, B=2, n0=4, n1=5, n2=6, mode=R, r=10, table=p, desc=None, ws=p, ws_bytes=big,
                offsets=p, capacity=10, rows=p, xyz=p, rgb16=p):
        return lib.sn_voxel_cloud_scatter(grid, dtype, B, n0, n1, n2, mode, r, table, desc, ws, ws_bytes, offsets, capacity,
                                          rows, xyz, rgb16, None)

    for call, required in ((count, ("grid", "ws", "offsets", "bad")), (scatter, ("grid", "ws", "offsets", "table"))):
        for name in required:
            assert call(**{name: None}) == -1, name
            assert b"null" in lib.sn_last_error()
        for kw in ({"B": 0}, {"B": -1}, {"n0": 0}, {"n1": -3}, {"n2": 0}):
            assert call(**kw) == -1, kw
            assert b"positive" in lib.sn_last_error()
        for r in (1, 0, -4, 33):
            assert call(r=r) == -1
            assert b"outside 2..32" in lib.sn_last_error()
        for mode in (2, -1):
            assert call(mode=mode) == -1
            assert b"mode" in lib.sn_last_error()
        for dtype in (_hip.SN_BF16, _hip.SN_I32, 17, -1):
            assert call(dtype=dtype) == -1
            assert b"dtype" in lib.sn_last_error()
        need = lib.sn_voxel_cloud_ws_bytes(2, 120)
        assert need == 8 * 2 * (3 * 1 + 1)
        assert call(ws_bytes=ctypes.c_size_t(need - 1)) == -1
        assert b"sn_voxel_cloud_ws_bytes" in lib.sn_last_error()
        for name in ("grid", "ws", "offsets"):
            assert call(**{name: off(4)}) == -1, name
            assert b"aligned" in lib.sn_last_error()
        assert call(grid=off(2), dtype=_hip.SN_F32) == -1, "an f32 grid is 4-byte aligned"
        assert call(mode=D, r=0, ws_bytes=ctypes.c_size_t(8)) == -1            # (r is not read in the density mode:
        assert b"sn_voxel_cloud_ws_bytes" in lib.sn_last_error()               # the next check is the one that refuses)
        assert call(desc=off(4)) == -1
        assert call(B=65536) == -2 and call(n0=2048, n1=1024, n2=1024) == -2
        assert b"beyond" in lib.sn_last_error()
    assert count(bad=off(4)) == -1
    assert scatter(rows=None, xyz=None) == -1
    assert b"neither" in lib.sn_last_error()
    assert scatter(capacity=-1) == -1
    assert b"capacity" in lib.sn_last_error()
    assert scatter(rows=off(8)) == -1 and scatter(xyz=off(4)) == -1 and scatter(rgb16=off(1)) == -1
    assert b"aligned" in lib.sn_last_error()


def test_ws_bytes_and_chunk_cells():
    lib = _hip.load()
    c = lib.sn_voxel_cloud_chunk_cells()
    assert c == _hip.voxel_cloud_chunk_cells() and c >= 64 and c % 64 == 0
    for B, V in ((0, 1), (-1, 1), (1, 0), (1, -2), (65536, 1), (1, 1 << 31)):
        assert lib.sn_voxel_cloud_ws_bytes(B, V) == 0, (B, V)
    assert lib.sn_voxel_cloud_ws_bytes(65535, (1 << 31) - 1) > 0
    for V, chunks in ((1, 1), (c, 1), (c + 1, 2), (3 * c + 17, 4)):
        assert lib.sn_voxel_cloud_ws_bytes(5, V) == 8 * 5 * (3 * chunks + 1)
    with pytest.raises(_hip.HipLibraryError):
        _hip.voxel_cloud_ws_bytes(0, 1)


def test_cpu_tensors_raise():
    g = torch.zeros(2, 4, 4, 4)
    with pytest.raises(sna.HipLibraryError, match="no CPU path"):
        sna.voxel_cloud(g)
    with pytest.raises(sna.HipLibraryError, match="no CPU path"):
        sna.voxel_cloud(g, "ranges")
    with pytest.raises(sna.HipLibraryError, match="no CPU path"):
        sna.voxel_cloud(g.numpy())
    with pytest.raises(sna.HipLibraryError, match="las=True"):
        sna.write_voxel_cloud_las("x.las", sna.VoxelCloud(g, None, None, g, g, "density"))


def test_plot_and_bad_mode_raise():
    g = np.zeros((4, 4, 4))
    with pytest.raises(NotImplementedError):
        sna.plot_voxelgrid(g)                       # plot=True is the reference's default
    with pytest.raises(NotImplementedError):
        sna.plot_voxelgrid(g, "ranges", plot=True)
    with pytest.raises(ValueError, match="color_mode"):
        sna.plot_voxelgrid(g, "coolwarm", plot=False)
    with pytest.raises(ValueError, match="color_mode"):
        sna.voxel_cloud(torch.zeros(1, 2, 2, 2), "coolwarm")
    with pytest.raises(TypeError):
        sna.plot_voxelgrid(g, plot=False, rr=5)
    with pytest.raises(ValueError):
        sna.plot_quantile_uncertainty(np.zeros((4, 4, 4)))
    with pytest.raises(ValueError):
        sna.plot_quantile_uncertainty(np.zeros((1, 4, 4, 4)))


def test_restatement_rules_that_are_build_defined():
    # rgb16: clamp(rint(v), 0, 255) * 257, NaN -> 0, halves to even
    v = np.array([[0.0, 255.0, 127.5], [128.5, -3.0, 300.0], [np.nan, 254.5, 0.49]])
    assert vc.rgb16(v).tolist() == [[0, 65535, 128 * 257], [128 * 257, 0, 65535], [0, 254 * 257, 0]]
    # bad: NaN kept, colours outside [0, 255]
    g = np.array([[[0.0, np.nan, 1.0], [1.5, -1.0, -1.25]]])
    assert vc.bad_counts(g, "density") == (1, 2) and vc.bad_counts(g, "ranges") == (0, 0)
    rows = vc.restate(g, "density")
    assert rows.shape == (5, 6) and rows[0, 3] == 255.0 and np.isnan(rows[0, 4]) and np.isnan(rows[0, 5])
