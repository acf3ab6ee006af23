"""Point rendering (K23), the part that needs no GPU: the oracle on images worked by hand, the two camera builders, the
PNG writer, the argument checks of the C entries, and every case builder's own assertions."""
import ctypes

import numpy as np
import pytest
import torch

import scene_net_amd as sna
from scene_net_amd import _hip

import render_cases as rc

BG = rc.BACKGROUND


def key(dq, j):
    return np.uint64((dq << 32) | j)


# ================================================================ the oracle, by hand
def test_nearest_wins_and_the_lowest_row_breaks_a_tie():
    # rows 0 and 1 on pixel (1, 1): row 1 is nearer; rows 2 and 3 on pixel (2, 0) at one depth: row 2 wins; row 4 alone
    P = [[1.5, 1.5, 0.75], [1.25, 1.75, 0.25], [2.5, 0.5, 0.5], [2.75, 0.25, 0.5], [0.0, 2.0, 0.0]]
    case = rc.one_tile(P, [rc.pixel_cam(1)], 3, 3)
    keys, count, bad = rc.splat_oracle(*case)
    want = np.full((3, 3), BG, dtype=np.uint64)
    want[1, 1] = key(1 << 30, 1)                  # 0.25 * 2^32
    want[0, 2] = key(1 << 31, 2)
    want[2, 0] = key(0, 4)
    assert np.array_equal(keys[0], want) and bad.tolist() == [0]
    assert count[0].tolist() == [[0, 0, 2], [0, 2, 0], [1, 0, 0]]
    rgb = np.arange(15, dtype=np.uint16).reshape(5, 3) * 1000 + 7
    rgba, index, depth = rc.resolve_oracle(keys, case.offsets, case.view_tile, rgb, rc.RGB16, (9, 8, 7, 6), 0.0)
    assert index[0].tolist() == [[-1, -1, 2], [-1, 1, -1], [4, -1, -1]]
    assert depth[0, 1, 1] == 1 << 30 and depth[0, 0, 0] == 2 ** 32 - 1
    assert rgba[0, 1, 1].tolist() == [3007 >> 8, 4007 >> 8, 5007 >> 8, 255], "the HIGH byte of the winner's words"
    assert rgba[0, 0, 0].tolist() == [9, 8, 7, 6]
    grey, _, _ = rc.resolve_oracle(keys, case.offsets, case.view_tile, None, rc.DEPTH, rc.WHITE, 0.0)
    assert grey[0, 1, 1].tolist() == [255 - 64, 255 - 64, 255 - 64, 255] and grey[0, 2, 0].tolist() == [255, 255, 255, 255]


def test_a_splat_is_clipped_at_a_corner_and_even_sizes_lean_right_and_down():
    # s = 3 centred on pixel (0, 0): -1 .. +1 clipped to 0 .. 1; s = 2 centred on (2, 2): 0 .. +1 clipped to 2 .. 2
    case = rc.one_tile([[0.5, 0.5, 0.5]], [rc.pixel_cam(3)], 3, 3)
    keys, count, _ = rc.splat_oracle(*case)
    assert (keys[0] != BG).tolist() == [[True, True, False], [True, True, False], [False, False, False]]
    assert count[0].tolist() == [[1, 0, 0], [0, 0, 0], [0, 0, 0]], "the centre pixel only"
    case = rc.one_tile([[2.5, 2.5, 0.5], [0.5, 1.5, 0.5]], [rc.pixel_cam(2)], 3, 3)
    keys, _, _ = rc.splat_oracle(*case)
    assert (keys[0] != BG).tolist() == [[False, False, False], [True, True, False], [True, True, True]]
    # a centre outside the image still reaches in; it is not counted
    case = rc.one_tile([[-0.5, 1.5, 0.5]], [rc.pixel_cam(3)], 3, 3)
    keys, count, _ = rc.splat_oracle(*case)
    assert (keys[0] != BG).tolist() == [[True, False, False]] * 3 and count.sum() == 0


def test_the_shade_of_one_pixel_by_hand():
    # centre at depth 0.75, left neighbour at 0.25, upper neighbour at 0.5, right neighbour farther (1 - 2^-32 ...), lower one
    # background: o = (0.75 - 0.25) * 2^32 + (0.75 - 0.5) * 2^32 = 0.75 * 2^32; shade = 1 / (1 + edl * 0.75)
    P = [[1.5, 1.5, 0.75], [0.5, 1.5, 0.25], [1.5, 0.5, 0.5], [2.5, 1.5, 0.875]]
    case = rc.one_tile(P, [rc.pixel_cam(1)], 3, 3)
    keys, _, _ = rc.splat_oracle(*case)
    assert keys[0, 2, 1] == BG
    rgb = np.array([[200 * 257, 100 * 257, 255 * 257]] * 4, dtype=np.uint16)
    for edl, shade in ((4.0, 0.25), (0.5, 1.0 / 1.375)):
        rgba, _, _ = rc.resolve_oracle(keys, case.offsets, case.view_tile, rgb, rc.RGB16, rc.WHITE, edl)
        want = [int(np.floor(c * shade + 0.5)) for c in (200, 100, 255)]
        assert rgba[0, 1, 1].tolist() == want + [255], (edl, rgba[0, 1, 1])
    rgba, _, _ = rc.resolve_oracle(keys, case.offsets, case.view_tile, rgb, rc.RGB16, rc.WHITE, 4.0)
    assert rgba[0, 1, 1].tolist() == [50, 25, 64, 255]
    # the nearest pixel has no nearer neighbour, and background neighbours contribute nothing: unshaded
    assert rgba[0, 1, 0].tolist() == [200, 100, 255, 255]
    # the upper one: its lower neighbour (the centre) is farther, the other three are background or outside
    assert rgba[0, 0, 1].tolist() == [200, 100, 255, 255]
    # the right one (0.875): left neighbour at 0.75 -> o = 0.125 * 2^32, shade = 1 / 1.5
    assert rgba[0, 1, 2].tolist() == [int(np.floor(c / 1.5 + 0.5)) for c in (200, 100, 255)] + [255]
    assert rgba[0, 2, 1].tolist() == list(rc.WHITE)
    # a lone pixel among background is unshaded whatever edl is
    lone = rc.one_tile([[1.5, 1.5, 0.99]], [rc.pixel_cam(1)], 3, 3)
    keys, _, _ = rc.splat_oracle(*lone)
    rgba, _, _ = rc.resolve_oracle(keys, lone.offsets, lone.view_tile, rgb, rc.RGB16, rc.WHITE, 1e6)
    assert rgba[0, 1, 1].tolist() == [200, 100, 255, 255]


def test_accumulate_form_of_the_oracle():
    a = rc.one_tile([[1.5, 1.5, 0.5]], [rc.pixel_cam(1)], 3, 3)
    b = rc.one_tile([[1.5, 1.5, 0.25], [0.5, 0.5, 0.5]], [rc.pixel_cam(1)], 3, 3)
    ka, ca, ba = rc.splat_oracle(*a)
    kb, cb, bb = rc.splat_oracle(*b)
    k2, c2, b2 = rc.splat_oracle(*b, keys=ka, count=ca, bad=ba)
    assert np.array_equal(k2, np.minimum(ka, kb)) and np.array_equal(c2, ca + cb) and b2.tolist() == [0]
    assert ka[0, 1, 1] == key(1 << 31, 0), "the given buffers are copied, not written"


# ================================================================ cameras
def corners(lo, hi):
    return np.array([[(lo, hi)[i][0], (lo, hi)[j][1], (lo, hi)[k][2]] for i in (0, 1) for j in (0, 1) for k in (0, 1)], dtype=np.float64)


def pixels(P, cam):
    """(px, py, d) by the literal sequence"""
    A = cam[:12].reshape(3, 4)
    x, y, z = P[:, 0], P[:, 1], P[:, 2]
    c = [((A[r, 0] * x + A[r, 1] * y) + A[r, 2] * z) + A[r, 3] for r in range(3)]
    return (c[0] / c[2], c[1] / c[2], c[2]) if cam[12] == 1.0 else tuple(c)


@pytest.mark.parametrize("view", ["top", "front", "side", (30.0, 20.0)])
@pytest.mark.parametrize("box", [((0.0, 0.0, 0.0), (10.0, 20.0, 5.0)), ((5.44e5, 4.634e6, 1.5e2), (5.4403e5, 4.63403e6, 2.1e2)),
                                 ((-3.0, -1.0, -2.0), (-1.0, 7.0, -2.0))])
def test_ortho_camera_fits_the_box(view, box):
    lo, hi = (np.array(v) for v in box)
    W, H = 320, 200
    cam = sna.ortho_camera(lo, hi, view, W, H, margin=0.02, point_size=3)
    assert cam.shape == (16,) and cam.dtype == np.float64 and cam[12] == 0.0 and cam[15] == 3.0 and rc.camera_ok(cam)
    C = corners(lo, hi)
    px, py, d = pixels(C, cam)
    assert np.all((px >= 0) & (px < W) & (py >= 0) & (py < H)), "the eight corners are inside the image"
    assert np.all((cam[13] <= d) & (d < cam[14])), "and between near and far"
    ok, _, ix, iy = rc.project(C, cam)
    assert ok.all()
    su, sv = np.linalg.norm(cam[0:3]), np.linalg.norm(cam[4:7])
    assert abs(su - sv) <= 1e-12 * su, "one scale on both axes"
    assert abs(cam[0:3] @ cam[4:7]) <= 1e-12 * su * sv and abs(np.linalg.norm(cam[8:11]) - 1.0) < 1e-15
    # the tighter axis fills the image up to the margin
    fill = max((px.max() - px.min()) / W, (py.max() - py.min()) / H)
    assert abs(fill - 0.96) < 1e-6


def test_top_view_has_north_up():
    lo, hi = np.array([100.0, 200.0, 0.0]), np.array([150.0, 250.0, 30.0])
    cam = sna.ortho_camera(lo, hi, "top", 256, 256)
    c = (lo + hi) / 2
    P = np.array([c, c + [1.0, 0, 0], c + [0, 1.0, 0], c + [0, 0, 1.0]])
    px, py, d = pixels(P, cam)
    assert px[1] > px[0] and py[1] == py[0], "+x goes to +u"
    assert py[2] < py[0] and px[2] == px[0], "+y goes to -v: north is up"
    assert d[3] < d[0] and px[3] == px[0] and py[3] == py[0], "a higher point is nearer"
    assert abs(px[0] - 128.0) < 1e-9 and abs(py[0] - 128.0) < 1e-9
    # front: from the south, +z up, farther north is farther; side: from the east, +y to the right
    px, py, d = pixels(P, sna.ortho_camera(lo, hi, "front", 256, 256))
    assert px[1] > px[0] and py[3] < py[0] and d[2] > d[0]
    px, py, d = pixels(P, sna.ortho_camera(lo, hi, "side", 256, 256))
    assert px[2] > px[0] and py[3] < py[0] and d[1] < d[0]
    # the named views are the (azimuth, elevation) family's members
    for name, ae in (("top", (-90.0, 90.0)), ("front", (-90.0, 0.0)), ("side", (0.0, 0.0))):
        assert np.allclose(sna.ortho_camera(lo, hi, name, 256, 256), sna.ortho_camera(lo, hi, ae, 256, 256), atol=1e-9)
    for bad in ({"view": "below"}, {"point_size": 0}, {"point_size": 10}, {"point_size": 1.5}, {"margin": 0.5}):
        kw = {"view": "top", **bad}
        with pytest.raises(ValueError):
            sna.ortho_camera(lo, hi, width=64, height=64, **kw)
    with pytest.raises(ValueError):
        sna.ortho_camera(hi, lo, "top", 64, 64)


def test_perspective_camera():
    eye, target = np.array([10.0, -20.0, 15.0]), np.array([12.0, 5.0, 3.0])
    W, H = 640, 480
    cam = sna.perspective_camera(eye, target, (0.0, 0.0, 1.0), 60.0, W, H, 0.5, 500.0, point_size=2)
    assert cam[12] == 1.0 and cam[13] == 0.5 and cam[14] == 500.0 and cam[15] == 2.0 and rc.camera_ok(cam)
    px, py, d = pixels(target[None], cam)
    assert abs(px[0] - W / 2) < 1e-9 and abs(py[0] - H / 2) < 1e-9, "the target is at the image centre"
    assert abs(d[0] - np.linalg.norm(target - eye)) < 1e-12, "depth is the distance along the view direction"
    # a point above the target is higher in the image (smaller y); one half the field of view up is on the top border
    px, py, _ = pixels((target + [0.0, 0.0, 1.0])[None], cam)
    assert py[0] < H / 2
    fwd = (target - eye) / np.linalg.norm(target - eye)
    right = np.cross(fwd, [0.0, 0.0, 1.0])
    right /= np.linalg.norm(right)
    upc = np.cross(right, fwd)
    edge = eye + 7.0 * (fwd + np.tan(np.radians(30.0)) * upc)
    px, py, _ = pixels(edge[None], cam)
    assert abs(py[0]) < 1e-9 and abs(px[0] - W / 2) < 1e-9
    # behind the eye and at the eye: rejected by the rule
    behind = np.array([eye - 3.0 * fwd, eye, eye + 0.25 * fwd, eye + 2.0 * fwd])
    ok, _, _, _ = rc.project(behind, cam)
    assert ok.tolist() == [False, False, False, True]
    keys, count, bad = rc.splat_oracle(*rc.one_tile(behind[:3], [cam], H, W))
    assert (keys == BG).all() and count.sum() == 0 and bad.tolist() == [0]
    for kw in ({"near": 0.0}, {"near": 5.0, "far": 5.0}, {"fov_y_deg": 180.0}):
        args = dict(fov_y_deg=60.0, width=W, height=H, near=0.5, far=500.0)
        args.update(kw)
        with pytest.raises(ValueError):
            sna.perspective_camera(eye, target, (0, 0, 1), **args)
    with pytest.raises(ValueError):
        sna.perspective_camera(eye, eye, (0, 0, 1), 60.0, W, H, 0.5, 500.0)
    with pytest.raises(ValueError):
        sna.perspective_camera(eye, eye + [0, 0, 1.0], (0, 0, 1), 60.0, W, H, 0.5, 500.0)


# ================================================================ PNG
@pytest.mark.parametrize("shape", [(1, 1), (7, 5), (257, 129)])
def test_png_bytes_round_trip(shape, tmp_path):
    H, W = shape
    img = np.random.default_rng(240 + H).integers(0, 256, (H, W, 4)).astype(np.uint8)
    data = sna.png_bytes(img)
    assert np.array_equal(rc.decode_png(data), img)
    assert np.array_equal(rc.decode_png(sna.png_bytes(torch.from_numpy(img))), img), "a host tensor serves too"
    path = str(tmp_path / "image.png")
    assert sna.write_png(path, img) == len(data) and open(path, "rb").read() == data
    for bad in (img[..., :3], img.astype(np.int32), img[0], np.zeros((0, 4, 4), dtype=np.uint8)):
        with pytest.raises(ValueError):
            sna.png_bytes(bad)


# ================================================================ the C entries' argument checks
def test_argument_checks_need_no_gpu():
    lib = _hip.load()
    assert lib.sn_render_chunk_points() == _hip.render_chunk_points() == 256
    assert (_hip.SN_RENDER_MAX_VIEWS, _hip.SN_RENDER_MAX_SPLAT) == (64, 9)
    buf = ctypes.create_string_buffer(512)
    base = (ctypes.addressof(buf) + 15) // 16 * 16
    p = ctypes.c_void_p(base)
    off = lambda d: ctypes.c_void_p(base + d)   # noqa: E731

    def splat(pts=p, offsets=p, total=100, B=2, cam=p, view_tile=p, K=3, H=16, W=16, flags=0, keys=p, count=p, bad_views=p):
        return lib.sn_render_splat(pts, offsets, total, B, cam, view_tile, K, H, W, flags, keys, count, bad_views, None)

    for name in ("pts", "offsets", "cam", "view_tile", "keys", "bad_views"):
        assert splat(**{name: None}) == -1, name
        assert b"null" in lib.sn_last_error() and name.encode() in lib.sn_last_error()
    for kw, word in (({"total": 0}, b"total"), ({"total": -3}, b"total"), ({"B": 0}, b"B must"), ({"B": -1}, b"B must"),
                     ({"K": 0}, b"K must"), ({"K": -2}, b"K must"), ({"H": 0}, b"H and W"), ({"W": 0}, b"H and W"),
                     ({"H": -5}, b"H and W"), ({"flags": 8}, b"flags"), ({"flags": -1}, b"flags"), ({"flags": 16 | 1}, b"flags"),
                     ({"flags": 2 | 4}, b"at once")):
        assert splat(**kw) == -1, kw
        assert word in lib.sn_last_error(), (kw, lib.sn_last_error())
    for kw, word in (({"K": 65}, b"SN_RENDER_MAX_VIEWS"), ({"H": 1 << 16, "W": 1 << 15}, b"2^31"),
                     ({"H": 46341, "W": 46341}, b"2^31"), ({"total": (1 << 33) + 1}, b"2^33"), ({"B": 65537}, b"65536")):
        assert splat(**kw) == -2, kw
        assert word in lib.sn_last_error(), (kw, lib.sn_last_error())
    for name, d in (("pts", 4), ("offsets", 4), ("cam", 4), ("keys", 4), ("view_tile", 2), ("count", 2), ("bad_views", 2)):
        assert splat(**{name: off(d)}) == -1, name
        assert b"aligned" in lib.sn_last_error()

    def resolve(keys=p, K=3, H=16, W=16, offsets=p, B=2, view_tile=p, rgb16=p, mode=0, background=0xffffffff, edl=0.0, rgba=p,
                index=p, depth_q=p):
        return lib.sn_render_resolve(keys, K, H, W, offsets, B, view_tile, rgb16, mode, background, edl, rgba, index, depth_q, None)

    for name in ("keys", "offsets", "view_tile", "rgba"):
        assert resolve(**{name: None}) == -1, name
        assert b"null" in lib.sn_last_error() and name.encode() in lib.sn_last_error()
    assert resolve(rgb16=None) == -1 and b"rgb16" in lib.sn_last_error(), "RGB16 mode needs the colours"
    for kw, word in (({"B": 0}, b"B must"), ({"K": 0}, b"K must"), ({"H": 0}, b"H and W"), ({"W": -1}, b"H and W"),
                     ({"mode": 2}, b"mode"), ({"mode": -1}, b"mode"), ({"edl": -0.5}, b"edl"), ({"edl": float("nan")}, b"edl"),
                     ({"edl": float("inf")}, b"edl")):
        assert resolve(**kw) == -1, kw
        assert word in lib.sn_last_error(), (kw, lib.sn_last_error())
    for kw, word in (({"K": 65}, b"SN_RENDER_MAX_VIEWS"), ({"H": 1 << 16, "W": 1 << 15}, b"2^31"), ({"B": 65537}, b"65536")):
        assert resolve(**kw) == -2, kw
        assert word in lib.sn_last_error(), (kw, lib.sn_last_error())
    for name, d in (("keys", 4), ("offsets", 4), ("index", 4), ("view_tile", 2), ("depth_q", 2), ("rgba", 2), ("rgb16", 1)):
        assert resolve(**{name: off(d)}) == -1, name
        assert b"aligned" in lib.sn_last_error()


def test_cpu_tensors_raise_and_names_are_exported():
    xyz = torch.zeros(8, 3, dtype=torch.float64)
    cam = sna.ortho_camera([0, 0, 0], [1, 1, 1], "top", 8, 8)
    grid = torch.zeros(1, 4, 4, 4)
    for call in (lambda: sna.render_points(xyz, cameras=cam, size=(8, 8)), lambda: sna.render_scan(xyz, size=(8, 8)),
                 lambda: sna.render_voxelgrid(grid), lambda: sna.render_pred_vs_gt(grid, grid, 0.5)):
        with pytest.raises(sna.HipLibraryError, match="no CPU path"):
            call()
    for name in ("RenderedViews", "ortho_camera", "perspective_camera", "render_points", "render_scan", "render_voxelgrid",
                 "render_pred_vs_gt", "png_bytes", "write_png"):
        assert hasattr(sna, name) and name in sna.__all__
    with pytest.raises(NotImplementedError):
        sna.plot_voxelgrid(np.zeros((2, 2, 2)), plot=True)           # unchanged: there is still no viewer
    table = sna.default_class_table(64)
    assert table.shape == (64, 3) and table.min() >= 0.0 and table.max() <= 1.0 and len(np.unique(table, axis=0)) == 64


# ================================================================ the cases
@pytest.mark.parametrize("name", rc.CASE_NAMES, ids=rc.case_id)
def test_case_builders_hold_their_own_assertions(name):
    case = rc.case(name)
    keys, count, bad = rc.oracle(name, case)
    K = len(case.cam)
    assert keys.shape == count.shape == (K, case.H, case.W) and bad.shape == (K,) and len(case.view_tile) == K
    assert case.offsets[0] == 0 and case.offsets[-1] == len(case.pts)
    assert (keys != BG).any(), "something is drawn"
    # count and keys agree on where an accepted centre fell, at s >= 1: a counted pixel is a foreground pixel
    assert not ((count > 0) & (keys == BG)).any()
