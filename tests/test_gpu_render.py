"""K23 on the GPU: sn_render_splat / sn_render_resolve and the layers above them against the numpy restatement of
tests/render_cases.py.  No tolerance anywhere: keys, counts, indices, depth quanta and pixel bytes are compared as integers.
Every output sits in a sentinel-filled buffer with guard slots behind it, the batch carries rows behind offsets[B] that would
draw if they were read, and every buffer is tried one element off a 16-byte boundary."""
import numpy as np
import pytest
import torch

import render_cases as rc
import scene_net_amd as sna
from scene_net_amd import _hip

pytestmark = pytest.mark.gpu

GUARD = 7                       # sentinel slots behind every output
BEYOND = 3                      # rows behind offsets[B], inside `total`
SENT_KEY = 0x5A5A5A5A5A5A5A5A
SENT_I32 = 0x5B5B5B5B
SENT_U8 = 0x5C


def shifted(arr, dev, shift):
    """The array on the device, `shift` elements into a larger buffer"""
    flat = torch.from_numpy(np.ascontiguousarray(arr)).reshape(-1)
    buf = torch.empty(flat.numel() + shift, dtype=flat.dtype, device=dev)
    view = buf[shift:]
    view.copy_(flat)
    return view.reshape(arr.shape)


def sentinel(n, value, dtype, dev, shift):
    return torch.full((n + GUARD + shift,), value, dtype=dtype, device=dev)[shift:]


class Batch:
    """A case's inputs on the device: BEYOND rows behind offsets[B] (in front of every identity camera: they would draw)"""

    def __init__(self, dev, case, shift=0):
        self.case, self.dev, self.shift = case, dev, shift
        extra = np.tile([[0.5, 0.5, 0.5]], (BEYOND, 1))
        self.pts = shifted(np.concatenate([case.pts, extra]), dev, shift)
        self.offsets = shifted(case.offsets, dev, shift)
        self.cam = shifted(case.cam, dev, 2 * shift)
        self.view_tile = shifted(case.view_tile, dev, shift)
        self.total = len(case.pts)
        self.rgb_host = rc.colours(self.total + BEYOND)
        self.rgb16 = shifted(self.rgb_host.view(np.int16), dev, shift)
        self.K, self.H, self.W = len(case.cam), case.H, case.W
        self.pixels = self.K * self.H * self.W


def run_splat(batch, into=None, want_count=True, look=None, dirty=False):
    """-> device (keys, count, bad) views of sentinel-backed buffers and numpy copies, guards checked"""
    dev, shift, n, K = batch.dev, batch.shift, batch.pixels, batch.K
    if into is None:
        keys = sentinel(n, SENT_KEY, torch.int64, dev, shift)
        count = sentinel(n, SENT_I32, torch.int32, dev, shift) if want_count else None
        bad = sentinel(K, SENT_I32, torch.int32, dev, shift)
        if dirty:
            keys[:n] = torch.randint(0, 1 << 40, (n,), device=dev)
            count[:n] = 77
            bad[:K] = 1
    else:
        keys, count, bad = into
    _hip.render_splat(batch.pts, batch.offsets, batch.cam, batch.view_tile, (batch.H, batch.W), keys[:n],
                      None if count is None else count[:n], bad[:K], accumulate=into is not None, look=look)
    torch.cuda.synchronize()
    k, b = keys.cpu().numpy().view(np.uint64), bad.cpu().numpy()
    assert np.all(k[n:] == SENT_KEY) and np.all(b[K:] == SENT_I32), "guard slots were touched"
    c = None
    if count is not None:
        c = count.cpu().numpy().view(np.uint32)
        assert np.all(c[n:] == SENT_I32), "guard slots were touched"
        c = c[:n].reshape(K, batch.H, batch.W)
    return (keys, count, bad), (k[:n].reshape(K, batch.H, batch.W), c, b[:K])


def run_resolve(batch, keys, mode, edl, background=rc.WHITE, want_index=True, want_depth=True):
    dev, shift, n = batch.dev, batch.shift, batch.pixels
    rgba = sentinel(4 * n, SENT_U8, torch.uint8, dev, 4 * shift)
    index = sentinel(n, SENT_KEY, torch.int64, dev, shift) if want_index else None
    depth = sentinel(n, SENT_I32, torch.int32, dev, shift) if want_depth else None
    _hip.render_resolve(keys[:n], (batch.H, batch.W), batch.offsets, batch.view_tile,
                        batch.rgb16 if mode == rc.RGB16 else None, mode, background, edl, rgba[:4 * n],
                        None if index is None else index[:n], None if depth is None else depth[:n])
    torch.cuda.synchronize()
    shape = (batch.K, batch.H, batch.W)
    r = rgba.cpu().numpy()
    assert np.all(r[4 * n:] == SENT_U8), "guard slots were touched"
    out = [r[:4 * n].reshape(shape + (4,)), None, None]
    if index is not None:
        i = index.cpu().numpy()
        assert np.all(i[n:] == SENT_KEY), "guard slots were touched"
        out[1] = i[:n].reshape(shape)
    if depth is not None:
        d = depth.cpu().numpy().view(np.uint32)
        assert np.all(d[n:] == SENT_I32), "guard slots were touched"
        out[2] = d[:n].reshape(shape)
    return out


def same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if not np.array_equal(got, want):
        at = np.argwhere(got != want)
        raise AssertionError(f"{what}: {len(at)} of {got.size} differ, first at {at[0].tolist()}: {got[tuple(at[0])]} != {want[tuple(at[0])]}")


# ================================================================ every case against the oracle
@pytest.mark.parametrize("name", rc.CASE_NAMES, ids=rc.case_id)
def test_splat_and_resolve_equal_the_oracle(hip_device, name):
    case = rc.case(name)
    exp = rc.oracle(name, case)
    dev_keys = None
    for shift, look, want_count in ((0, None, True), (0, True, True), (1, False, True), (1, None, False)):
        batch = Batch(hip_device, case, shift)
        bufs, (keys, count, bad) = run_splat(batch, want_count=want_count, look=look)
        same(keys, exp[0], f"keys (shift {shift}, look {look})")
        same(bad, exp[2], "bad_views")
        if want_count:
            same(count, exp[1], "count")
        dev_keys = bufs[0]
    # (the last batch, one element off the boundary, serves the resolve)
    for mode in (rc.RGB16, rc.DEPTH):
        for edl in rc.EDLS:
            want = rc.resolve_oracle(exp[0], case.offsets, case.view_tile, batch.rgb_host, mode, (1, 2, 3, 4), edl)
            got = run_resolve(batch, dev_keys, mode, edl, (1, 2, 3, 4))
            for g, w, what in zip(got, want, ("rgba", "index", "depth_q")):
                same(g, w, f"{what} (mode {mode}, edl {edl})")
    want = rc.resolve_oracle(exp[0], case.offsets, case.view_tile, batch.rgb_host, rc.RGB16, rc.WHITE, 0.5)
    for want_index, want_depth in ((False, True), (True, False), (False, False)):
        got = run_resolve(batch, dev_keys, rc.RGB16, 0.5, want_index=want_index, want_depth=want_depth)
        same(got[0], want[0], "rgba")
        assert (got[1] is None) == (not want_index) and (got[2] is None) == (not want_depth)
        if want_index:
            same(got[1], want[1], "index")
        if want_depth:
            same(got[2], want[2], "depth_q")


# ================================================================ accumulate, dirty buffers
def test_accumulate_composites_and_a_plain_call_clears(hip_device):
    a, b = rc.case(("ties",)), rc.case(("splats",))
    # the second layer: the splats case's rows through the first layer's two cameras, on its 16 x 16 images
    layer = rc.one_tile(b.pts * np.array([1.5, 1.0, 1.0]), a.cam, a.H, a.W)
    ea, eb = rc.oracle(("ties",), a), rc.splat_oracle(*layer)
    assert (eb[0] < ea[0]).any() and (ea[0] < eb[0]).any(), "each layer wins somewhere"
    first, second = Batch(hip_device, a), Batch(hip_device, layer, shift=1)
    bufs, _ = run_splat(first)
    _, (keys, count, bad) = run_splat(second, into=bufs)
    same(keys, np.minimum(ea[0], eb[0]), "keys")
    same(count, ea[1] + eb[1], "count")
    same(bad, np.zeros(2, dtype=np.int32), "bad_views")
    k2, c2, b2 = rc.splat_oracle(*layer, keys=ea[0], count=ea[1], bad=ea[2])
    same(keys, k2, "keys against the oracle's accumulate form")
    same(count, c2, "count against the oracle's accumulate form")
    # bad_views is composited too: a bad camera in the first call stays marked
    bad_first = rc.one_tile(a.pts, [a.cam[0], rc.pixel_cam(0)], a.H, a.W)
    bufs, (_, _, bad) = run_splat(Batch(hip_device, bad_first))
    assert bad.tolist() == [0, 1]
    _, (keys, _, bad) = run_splat(second, into=bufs)
    assert bad.tolist() == [0, 1]
    same(keys[1], eb[0][1], "the second layer alone on the image the bad camera left as background")
    # a plain call on dirty buffers equals one on fresh buffers
    _, (keys, count, bad) = run_splat(first, dirty=True)
    same(keys, ea[0], "keys")
    same(count, ea[1], "count")
    same(bad, ea[2], "bad_views")


# ================================================================ capture
def test_a_captured_graph_follows_the_cameras(hip_device):
    dev = hip_device
    case = rc.case(("shapes", 7, 5, 3))
    batch = Batch(dev, case)
    n, K, H, W = batch.pixels, batch.K, batch.H, batch.W
    keys = torch.empty(n, dtype=torch.int64, device=dev)
    count = torch.empty(n, dtype=torch.int32, device=dev)
    bad = torch.empty(K, dtype=torch.int32, device=dev)
    rgba = torch.empty(4 * n, dtype=torch.uint8, device=dev)
    index = torch.empty(n, dtype=torch.int64, device=dev)
    depth = torch.empty(n, dtype=torch.int32, device=dev)

    def launch():
        _hip.render_splat(batch.pts, batch.offsets, batch.cam, batch.view_tile, (H, W), keys, count, bad)
        _hip.render_resolve(keys, (H, W), batch.offsets, batch.view_tile, batch.rgb16, rc.RGB16, rc.WHITE, 0.5, rgba, index, depth)

    launch()                                                     # (eager first: the kernels are loaded)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch()
    # three camera sets: the case's own; view 1 with another point size and a flipped depth; view 0 made bad
    cams = [case.cam.copy() for _ in range(3)]
    cams[1][1, 15] = 4.0
    cams[1][1, 8:12] = -cams[1][1, 8:12]
    cams[1][1, 13], cams[1][1, 14] = -2.0, 0.5
    cams[2][0, 12] = 3.0
    rows = [None, 1, 0]
    seen = []
    for step, row in enumerate(rows):
        if row is not None:
            batch.cam[row].copy_(torch.from_numpy(cams[step][row]))        # a one-row copy between replays
        graph.replay()
        torch.cuda.synchronize()
        cam_now = cams[0].copy()
        for s in range(1, step + 1):
            cam_now[rows[s]] = cams[s][rows[s]]
        ek, ec, eb = rc.splat_oracle(case.pts, case.offsets, cam_now, case.view_tile, H, W)
        er, ei, ed = rc.resolve_oracle(ek, case.offsets, case.view_tile, batch.rgb_host, rc.RGB16, rc.WHITE, 0.5)
        same(keys.cpu().numpy().view(np.uint64).reshape(K, H, W), ek, f"keys, replay {step}")
        same(count.cpu().numpy().view(np.uint32).reshape(K, H, W), ec, f"count, replay {step}")
        same(bad.cpu().numpy(), eb, f"bad_views, replay {step}")
        same(rgba.cpu().numpy().reshape(K, H, W, 4), er, f"rgba, replay {step}")
        same(index.cpu().numpy().reshape(K, H, W), ei, f"index, replay {step}")
        same(depth.cpu().numpy().view(np.uint32).reshape(K, H, W), ed, f"depth_q, replay {step}")
        seen.append(ek.tobytes())
    assert len(set(seen)) == 3, "the three camera sets give three images"


# ================================================================ the layers above
def views_equal(a, b):
    for name in ("rgba", "index", "depth_q", "count", "keys", "bad_views"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name


def test_render_points_against_the_oracle_and_into(hip_device):
    dev = hip_device
    case = rc.case(("ties",))
    rgb = rc.colours(len(case.pts))
    xyz = torch.from_numpy(case.pts).to(dev)
    rgb16 = torch.from_numpy(rgb.view(np.int16)).to(dev).view(torch.uint16)
    out = sna.render_points(xyz, rgb16, cameras=case.cam, size=(case.H, case.W), edl=0.5, background=(1, 2, 3, 4))
    ek, ec, eb = rc.oracle(("ties",), case)
    er, ei, ed = rc.resolve_oracle(ek, case.offsets, case.view_tile, rgb, rc.RGB16, (1, 2, 3, 4), 0.5)
    assert out.K == 2 and out.size == (16, 16) and out.layer is None
    same(out.keys.cpu().numpy().view(np.uint64), ek, "keys")
    same(out.count.cpu().numpy().view(np.uint32), ec, "count")
    same(out.rgba.cpu().numpy(), er, "rgba")
    same(out.index.cpu().numpy(), ei, "index")
    same(out.depth_q.cpu().numpy().view(np.uint32), ed, "depth_q")
    out.check()
    assert np.array_equal(rc.decode_png(out.png(1)), er[1])
    # the depth as a grey when there are no colours
    grey = sna.render_points(xyz, cameras=case.cam, size=(case.H, case.W))
    same(grey.rgba.cpu().numpy(), rc.resolve_oracle(ek, case.offsets, case.view_tile, None, rc.DEPTH, rc.WHITE, 0.0)[0], "grey")
    # a second layer with another point size over the first
    layer = rc.case(("splats",)).pts[::5] * np.array([1.5, 1.0, 1.0])
    lrgb = rc.colours(len(layer), seed=236)
    cams2 = case.cam.copy()
    cams2[:, 15] = 4.0
    both = sna.render_points(torch.from_numpy(layer).to(dev), torch.from_numpy(lrgb.view(np.int16)).to(dev).view(torch.uint16),
                             cameras=cams2, edl=0.5, background=(1, 2, 3, 4), size=(case.H, case.W), into=out)
    lk, lc, _ = rc.splat_oracle(layer, np.array([0, len(layer)]), cams2, case.view_tile, case.H, case.W, keys=ek, count=ec, bad=eb)
    lr, li, ld = rc.resolve_oracle(lk, np.array([0, len(layer)]), case.view_tile, lrgb, rc.RGB16, (1, 2, 3, 4), 0.5)
    won = lk != ek
    assert won.any() and (~won & (ek != rc.BACKGROUND)).any()
    same(both.keys.cpu().numpy().view(np.uint64), lk, "keys")
    same(both.count.cpu().numpy().view(np.uint32), lc, "count")
    same(both.rgba.cpu().numpy(), np.where(won[..., None], lr, er), "rgba")
    same(both.index.cpu().numpy(), np.where(won, li, ei), "index")
    same(both.layer.cpu().numpy(), won.astype(np.int32), "layer")
    same(out.keys.cpu().numpy().view(np.uint64), ek, "`into` is left as it was")
    # a bad camera is counted, and check() raises on it
    bad = case.cam.copy()
    bad[1, 15] = 0.0
    res = sna.render_points(xyz, rgb16, cameras=bad, size=(case.H, case.W))
    assert res.bad_views.cpu().tolist() == [0, 1]
    with pytest.raises(ValueError, match=r"views \[1\]"):
        res.check()
    with pytest.raises(sna.HipLibraryError, match="no CPU path"):
        sna.render_points(xyz.cpu(), cameras=case.cam, size=(8, 8))
    with pytest.raises(sna.HipLibraryError, match="no CPU path"):
        sna.render_points(xyz, rgb16.cpu(), cameras=case.cam, size=(8, 8))


def test_render_scan_is_class_colors_plus_render_points(hip_device, tmp_path):
    dev = hip_device
    rng = np.random.default_rng(237)
    P = np.array([5.44e5, 4.634e6, 1.5e2]) + rng.random((1000, 3)) * np.array([30.0, 20.0, 40.0])
    classes = rng.integers(0, 6, 1000).astype(np.float64)
    xyz, cls = torch.from_numpy(P).to(dev), torch.from_numpy(classes).to(dev)
    out = sna.render_scan(xyz, classes=cls, size=(48, 64), edl=2.0, point_size=2)
    cams = np.stack([sna.ortho_camera(P.min(axis=0), P.max(axis=0), v, 64, 48, 0.02, 2) for v in ("top", "front", "side")])
    rgb = sna.class_colors(cls, sna.default_class_table(), las=True).rgb
    hand = sna.render_points(xyz, rgb, cameras=cams, size=(48, 64), edl=2.0)
    views_equal(out, hand)
    out.check()
    keys, count, _ = rc.splat_oracle(P, np.array([0, 1000]), cams, np.zeros(3, dtype=np.int32), 48, 64)
    same(out.keys.cpu().numpy().view(np.uint64), keys, "keys")
    assert count.sum() == 3000, "every point is inside every view"
    assert len(np.unique(out.rgba.cpu().numpy().reshape(-1, 4), axis=0)) > 6
    path = str(tmp_path / "top.png")
    sna.write_png(path, out.rgba[0])
    assert np.array_equal(rc.decode_png(open(path, "rb").read()), out.rgba[0].cpu().numpy())
    # given colours, and none
    views_equal(sna.render_scan(xyz, rgb16=rgb, views=("side",), size=(48, 64), point_size=2),
                sna.render_points(xyz, rgb, cameras=cams[2:], size=(48, 64)))
    views_equal(sna.render_scan(xyz, views=[(30.0, 20.0)], size=(32, 32)),
                sna.render_points(xyz, cameras=sna.ortho_camera(P.min(axis=0), P.max(axis=0), (30.0, 20.0), 32, 32), size=(32, 32)))
    with pytest.raises(sna.HipLibraryError, match="no CPU path"):
        sna.render_scan(xyz.cpu())


def test_render_voxelgrid_and_pred_vs_gt_are_voxel_cloud_plus_render_points(hip_device):
    dev = hip_device
    rng = np.random.default_rng(238)
    grids = np.where(rng.random((2, 16, 16, 16)) < 0.05, rng.random((2, 16, 16, 16)) * 2.0 - 1.0, 0.0)
    g = torch.from_numpy(grids).to(dev)
    out = sna.render_voxelgrid(g, "density", views=("top", "side"), size=(64, 80))
    cloud = sna.voxel_cloud(g, "density", las=True)
    cam = [sna.ortho_camera([-0.5] * 3, [15.5] * 3, v, 80, 64) for v in ("top", "side")]
    scale = np.linalg.norm(cam[0][:3])
    assert abs(scale - 0.96 * 64 / 16) < 1e-9
    for c in cam:
        c[15] = 4.0                                               # ceil(3.84): one voxel, one splat
    hand = sna.render_points(cloud.xyz, cloud.rgb, cloud.offsets, np.stack(cam + cam), [0, 0, 1, 1], (64, 80))
    views_equal(out, hand)
    out.check()
    assert out.K == 4 and (out.index[:2] < cloud.offsets[1]).all() and (out.index[2:][out.index[2:] >= 0] >= cloud.offsets[1]).all()
    keys, _, _ = rc.splat_oracle(cloud.xyz.cpu().numpy(), cloud.offsets.cpu().numpy(), np.stack(cam + cam), [0, 0, 1, 1], 64, 80)
    same(out.keys.cpu().numpy().view(np.uint64), keys, "keys")
    assert np.array_equal(rc.decode_png(sna.png_bytes(out.rgba[3])), out.rgba[3].cpu().numpy())
    assert sna.render_voxelgrid(torch.zeros_like(g)) is None
    # with the voxelisation's descriptor: scan coordinates, the box its lo .. hi, a voxel the first step of its edge tables;
    # n-mode (16 voxels of 2.5 / 5 / 1.25 along x / y / z) and size-mode (voxels of 2 in tables padded to 16)
    n_mode = np.concatenate([[100.0, 200.0, 10.0, 140.0, 280.0, 30.0], np.linspace(100.0, 140.0, 17), np.linspace(200.0, 280.0, 17),
                             np.linspace(10.0, 30.0, 17)])
    sized = np.concatenate([[0.0, 0.0, 0.0, 20.0, 24.0, 32.0], np.r_[np.arange(11) * 2.0, [np.inf] * 6],
                            np.r_[np.arange(13) * 2.0, [np.inf] * 4], np.arange(17) * 2.0])
    desc = torch.from_numpy(np.stack([n_mode, sized])).to(dev)
    own = g.clone()
    own[1, :, 10:, :] = 0.0                                       # (the padding cells of the size-mode tile hold nothing)
    own[1, :, :, 12:] = 0.0
    dout = sna.render_voxelgrid(own, "density", views=("front",), desc=desc, size=(64, 80))
    dcloud = sna.voxel_cloud(own, "density", desc=desc, las=True)
    c0 = sna.ortho_camera(n_mode[:3], n_mode[3:6], "front", 80, 64)
    c1 = sna.ortho_camera(sized[:3], sized[3:6], "front", 80, 64)
    s0, s1 = np.linalg.norm(c0[:3]), np.linalg.norm(c1[:3])
    assert abs(s0 - 0.96 * 80 / 40) < 1e-9 and abs(s1 - 0.96 * 64 / 32) < 1e-9
    c0[15], c1[15] = 9.0, 4.0                                    # ceil(1.92 * 5) = 10, kept at 9; ceil(1.92 * 2) = 4
    views_equal(dout, sna.render_points(dcloud.xyz, dcloud.rgb, dcloud.offsets, np.stack([c0, c1]), [0, 1], (64, 80)))
    dout.check()
    assert (dout.count.sum(dim=(1, 2)).cpu() == (dcloud.offsets[1:] - dcloud.offsets[:-1]).cpu()).all(), "every voxel is inside its image"
    # prediction against ground truth: the reference's (4 pred + gt) / 5 under the 'ranges' colours
    pred = torch.from_numpy(rng.random((1, 16, 16, 16))).to(dev)
    gt = torch.from_numpy((rng.random((1, 16, 16, 16)) < 0.3).astype(np.float64)).to(dev)
    pvg = sna.render_pred_vs_gt(pred, gt, 0.7, views=("front",), size=(64, 64))
    common = (4 * sna.prob_to_label(pred, 0.7) + gt) / 5
    assert sorted(torch.unique(common).cpu().tolist()) == [0.0, 0.2, 0.8, 1.0]
    ccloud = sna.voxel_cloud(common, "ranges", las=True)
    fcam = sna.ortho_camera([-0.5] * 3, [15.5] * 3, "front", 64, 64)
    fcam[15] = 4.0
    views_equal(pvg, sna.render_points(ccloud.xyz, ccloud.rgb, ccloud.offsets, fcam, [0], (64, 64)))
    assert len(np.unique(pvg.rgba.cpu().numpy().reshape(-1, 4), axis=0)) == 4, "hit, false alarm, miss and background"
    assert np.array_equal(rc.decode_png(pvg.png(0)), pvg.rgba[0].cpu().numpy())
    for call in (lambda: sna.render_voxelgrid(g.cpu()), lambda: sna.render_pred_vs_gt(pred.cpu(), gt, 0.5),
                 lambda: sna.render_pred_vs_gt(pred, gt.cpu(), 0.5)):
        with pytest.raises(sna.HipLibraryError, match="no CPU path"):
            call()
