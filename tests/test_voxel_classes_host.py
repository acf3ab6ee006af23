"""K18 on the CPU: the two formulations of the class grid against each other and against the reference's pandas lines, the
colour oracle against the golden file the reference wrote, the key map's order, the seeded table of color_pointcloud and the
argument checks of every new entry (no GPU is touched)."""
import ctypes

import numpy as np
import pytest

import binning_cases as bc
import voxel_classes_cases as kc
from scene_net_amd import _hip
from scene_net_amd.voxel_classes import random_class_colors


def grid_cases():
    """(name, dims, flat, labels): foreign points of a 5x7x3 and an 8x12x4 table with special labels, a cloud of its own
    64^3 grid, and one voxel that holds only NaN labels next to one that holds everything."""
    rng = np.random.default_rng(18)
    cases = []
    for dims in ((5, 7, 3), (8, 12, 4)):
        desc, _ = bc.host_desc("own", dims, 1)
        pts = bc.foreign_points(desc[0, :3], desc[0, 3:6], dims, rng, 1500)
        cases.append((f"foreign{dims}", dims, bc.expected_flat(desc[0], dims, pts), kc.special_labels(len(pts), rng)))
    pts = kc.cube_tile(3000, 5)
    dims = (64, 64, 64)
    cases.append(("own64", dims, bc.expected_flat(kc.own_desc(pts, dims), dims, pts), bc.LABELS[rng.integers(0, 4, 3000)]))
    flat = np.array([3, 3, 3, 9, 9, 9, 9, -1, 11, 11])
    lab = np.array([np.nan, np.nan, np.nan, -np.inf, np.nan, 5e-324, -2.0, 99.0, -np.inf, np.nan])
    cases.append(("by_hand", (5, 7, 3), flat, lab))
    return cases


@pytest.mark.parametrize("case", grid_cases(), ids=lambda c: c[0])
def test_grid_formulations_agree(case):
    _, dims, flat, lab = case
    a, b = kc.grid_pandas(flat, lab, dims), kc.grid_fmax(flat, lab, dims)
    assert a.shape == (dims[2], dims[0], dims[1])
    assert np.array_equal(kc.bits(a), kc.bits(b))
    assert (flat >= 0).sum() > 0 and np.count_nonzero(a) > 0


def test_grid_rules_by_hand():
    _, dims, flat, lab = grid_cases()[-1]
    g = kc.grid_fmax(flat, lab, dims).reshape(-1)
    assert np.isnan(g[3])                                   # only NaN labels
    assert g[9] == 5e-324                                   # NaN skipped; a denormal beats -inf and -2
    assert g[11] == -np.inf                                 # -inf is a value like any other
    assert g[0] == 0.0 and not np.signbit(g[0])             # nothing fell: np.zeros
    assert np.count_nonzero(g) == 3 and not (g == 99.0).any()       # the unbinned row takes no part


def test_key_map_is_strictly_monotone():
    tiny = 5e-324
    v = np.array([-np.inf, -1.7976931348623157e308, -1e300, -2.0, -1.0, -2.2250738585072014e-308, -1e-310, -tiny, -0.0, 0.0,
                  tiny, 1e-310, 2.2250738585072014e-308, 0.5, 1.0, 15.0, 65535.0, 1e300, 1.7976931348623157e308, np.inf])
    assert np.all(np.diff(v[v != 0]) > 0)                   # the vector itself is sorted
    k = kc.key_of(v)
    assert k.dtype == np.uint64
    assert np.all(k[1:] > k[:-1]), "strictly monotone, -0.0 below +0.0"
    assert int(k[0]) == 0x000FFFFFFFFFFFFF and int(k.min()) == int(k[0])       # -inf: the smallest key of a value
    assert not np.isin(k, np.array([0, 1], dtype=np.uint64)).any()             # 0 and 1 stay free: empty, NaN only
    rng = np.random.default_rng(3)
    r = rng.standard_normal(4000) * 10.0 ** rng.integers(-300, 300, 4000)
    order = np.argsort(r, kind="stable")
    assert np.all(np.diff(kc.key_of(r[order]).astype(object)) >= 0) and kc.key_of(r).min() > 1


def test_colour_oracle_equals_the_golden():
    gold = np.load(kc.GOLDEN)
    cases = kc.golden_cases()
    assert [c[0] for c in cases] == list(gold["names"]) and len(cases) == 6
    seen = set()
    for name, classes, table in cases:
        assert np.array_equal(gold[name + "_classes"], classes) and gold[name + "_classes"].dtype == classes.dtype
        assert np.array_equal(kc.bits(gold[name + "_table"]), kc.bits(table))
        want = gold[name + "_colors"]
        assert want.shape == (len(classes), 3)
        assert np.array_equal(kc.bits(kc.colors_loop(classes, table)), kc.bits(want)), name
        mine, unique, bad, short = kc.expected_colors(classes, table)
        assert np.array_equal(kc.bits(mine), kc.bits(want)) and bad == 0 and short == 0, name
        assert np.array_equal(unique, np.unique(classes))
        seen.add(len(unique))
    assert {1, 22} <= seen and 65535.0 in gold["kitti16_classes"] and 255.0 in gold["las_classes"]


def test_colour_oracle_where_the_reference_raises():
    table = np.arange(9.0).reshape(3, 3) / 10
    for classes in (np.array([1.0, np.nan, 2.0]), np.array([1.0, 2.0, 3.0, 4.0])):
        with pytest.raises(IndexError):
            kc.colors_loop(classes, table)
    mine, unique, bad, short = kc.expected_colors(np.array([1.0, np.nan, 2.5, -1.0, 65536.0, 7.0]), table)
    assert bad == 4 and short == 0 and unique.tolist() == [1.0, 7.0]
    assert np.isnan(mine[1:5]).all() and mine[0].tolist() == [0.0, 0.1, 0.2] and mine[5].tolist() == [0.3, 0.4, 0.5]
    mine, unique, bad, short = kc.expected_colors(np.array([1.0, 2.0, 3.0, 4.0, 4.0]), table)
    assert bad == 0 and short == 2 and np.isnan(mine[3:]).all() and not np.isnan(mine[:3]).any()
    assert kc.rgb16(np.array([[0.0, 1.0, 0.5], [np.nan, -0.2, 1.7], [1 / 255, 0.4980392156862745, 0.2]])).tolist() == \
        [[0, 65535, 128 * 257], [0, 0, 65535], [257, 127 * 257, 51 * 257]]


def test_seeded_table_is_the_reference_call():
    np.random.seed(1234)
    want = np.random.choice(256, size=(7, 3)) / 255
    np.random.seed(1234)
    got = random_class_colors(7)
    assert got.shape == (7, 3) and got.dtype == np.float64 and np.array_equal(kc.bits(got), kc.bits(want))
    assert got.min() >= 0.0 and got.max() <= 1.0


def test_argument_checks_need_no_gpu():
    lib = _hip.load()
    buf = ctypes.create_string_buffer(256)
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert p.value % 8 == 0
    off = lambda k: ctypes.c_void_p(p.value + k)   # noqa: E731

    def grid(pts=p, labels=p, offsets=p, total=100, B=2, desc=p, dims=(4, 4, 4), flags=0, out=p, unbinned=p, nan_labels=p):
        return lib.sn_voxel_classes(pts, labels, offsets, total, B, desc, *dims, flags, out, unbinned, nan_labels, None)

    def census(classes=p, offsets=p, total=100, B=2, present=p, bad=p):
        return lib.sn_class_census(classes, offsets, total, B, present, bad, None)

    def paint(classes=p, offsets=p, total=100, B=2, present=p, table=p, T=3, colors=p, rgb=p, unique=p, U_max=4, n_unique=p,
              short_table=p):
        return lib.sn_class_paint(classes, offsets, total, B, present, table, T, colors, rgb, unique, U_max, n_unique,
                                  short_table, None)

    for call, required in ((grid, ("pts", "labels", "offsets", "desc", "out", "unbinned", "nan_labels")),
                           (census, ("classes", "offsets", "present", "bad")),
                           (paint, ("classes", "offsets", "present", "table", "n_unique", "short_table"))):
        for name in required:
            assert call(**{name: None}) == -1, name
            assert b"null" in lib.sn_last_error(), name
            assert call(**{name: off(4 if name != "present" else 2)}) == -1, name
            assert b"aligned" in lib.sn_last_error(), name
        for kw in (dict(total=0), dict(total=-5), dict(B=0), dict(B=-1)):
            assert call(**kw) == -1, kw
        assert call(total=(1 << 33) + 1) == -2 and call(B=(1 << 16) + 1) == -2
    assert grid(dims=(4, 0, 4)) == -1 and grid(flags=2) == -1 and grid(flags=1 << 8) == -1
    assert grid(dims=(4000, 4000, 400)) == -2 and b"LDS" in lib.sn_last_error()
    assert grid(dims=(2048, 2048, 512)) == -2 and b"2^31" in lib.sn_last_error()
    assert paint(colors=None, rgb=None) == -1 and b"neither" in lib.sn_last_error()
    assert paint(T=0) == -1 and paint(U_max=0) == -1
    for name, k in (("colors", 4), ("unique", 4), ("rgb", 1)):
        assert paint(**{name: off(k)}) == -1, name
        assert b"aligned" in lib.sn_last_error()
    c, k = lib.sn_voxel_classes_chunk_points(), lib.sn_class_chunk_points()
    assert c == _hip.voxel_classes_chunk_points() and c >= 64 and c % 64 == 0
    assert k == _hip.class_chunk_points() and k >= 256 and k % 256 == 0
    assert _hip.SN_CLASS_WORDS * 32 == 65536
