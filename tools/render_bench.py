#!/usr/bin/env python3
"""K23 on one synthetic scan of 10^7 points (the crops bench's) and on the C2 batch (32 tiles of 10^5 points).  Timed
between HIP events after a warm-up, eager and captured into a hipGraph and replayed.
Splat: sn_render_splat (the clearing launch and the pass over the rows) at 1024 x 1024 with 1 and 3 orthographic views, one
perspective view, point sizes 1 and 3; as the library sends it (the look before the atomic where the point size is >= 2),
with the look at every size (SN_RENDER_LOOK_ALWAYS), with none (SN_RENDER_NO_LOOK), and without the count image.  Resolve:
sn_render_resolve with every output, shading off and on.
Yardstick, measured in the same run: sn_crop_count over the same rows with one box region -- the same 24 B per point read
once.  The mark is that time plus 25 %; the splat's position is reported INSIDE or OUTSIDE whichever it is.
Baselines that need none of this library's kernels: the same image through torch on the device (the projection as
elementwise fp64 and scatter_reduce(amin) on the keys) and the copy down plus a matplotlib scatter on the host, timed on
10^5 points and SCALED linearly.
The bench checks what it times: the keys against the torch formulation, bit for bit.  Writes one JSON file.
    python tools/render_bench.py --out profiles/render_bench.json [--iters 10]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from crops_bench import HBM_PEAK, synthetic_scan, timed  # noqa: E402
from voxel_classes_bench import ALLOWANCE, both_ways, verdict  # noqa: E402
import scene_net_amd as sna  # noqa: E402
from scene_net_amd import _hip  # noqa: E402
from scene_net_amd.synthetic import synthetic_tile  # noqa: E402

SIGN = -(1 << 63)


def torch_keys(pts, cam, H, W):
    """[H * W] int64 holding the u64 keys of one view of the rows pts by the rule in torch ops"""
    c = [float(v) for v in cam]
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    c0, c1, d = (((c[4 * r] * x + c[4 * r + 1] * y) + c[4 * r + 2] * z) + c[4 * r + 3] for r in range(3))
    px, py = (c0 / d, c1 / d) if c[12] == 1.0 else (c0, c1)
    ok = (d >= c[13]) & (d < c[14]) & (px.abs() < 2.0 ** 30) & (py.abs() < 2.0 ** 30)
    dq = torch.floor(((d - c[13]) / (c[14] - c[13])) * 4294967296.0).clamp_(0, 4294967295.0).to(torch.int64)
    ix, iy = torch.floor(px).to(torch.int64), torch.floor(py).to(torch.int64)
    j = torch.arange(pts.shape[0], device=pts.device, dtype=torch.int64)
    key = ((dq << 32) | j) ^ SIGN                       # (the sign bit flipped: unsigned order as signed order)
    out = torch.full((H * W,), (1 << 63) - 1, dtype=torch.int64, device=pts.device)
    s = int(c[15])
    for dy in range(-((s - 1) // 2), s // 2 + 1):
        for dx in range(-((s - 1) // 2), s // 2 + 1):
            X, Y = ix + dx, iy + dy
            m = ok & (X >= 0) & (X < W) & (Y >= 0) & (Y < H)
            out.scatter_reduce_(0, (Y * W + X)[m], key[m], "amin", include_self=True)
    return out ^ SIGN


def host_scatter(xyz_dev, rgb_dev, m):
    """seconds: (the copy down of m points, a matplotlib 3-D scatter of them rendered to a PNG in memory)"""
    import io
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    xyz = xyz_dev[:m].cpu().numpy()
    rgb = (rgb_dev[:m].cpu().view(torch.int16).numpy().view(np.uint16) >> 8) / 255.0
    d2h = time.perf_counter() - t0
    t0 = time.perf_counter()
    fig = plt.figure(figsize=(10.24, 10.24), dpi=100)
    ax = fig.add_subplot(projection="3d")
    ax.scatter(xyz[:, 0], xyz[:, 1], xyz[:, 2], c=rgb, s=1)
    fig.savefig(io.BytesIO(), format="png")
    plt.close(fig)
    return d2h, time.perf_counter() - t0


def case(name, pts, offsets, rgb16, cams, view_tile, args, yard, check_views=1):
    dev = pts.device
    H = W = args.size
    K = len(cams)
    cam = torch.from_numpy(np.stack(cams)).to(dev)
    vt = torch.tensor(view_tile, dtype=torch.int32, device=dev)
    keys = torch.empty((K, H, W), dtype=torch.int64, device=dev)
    count = torch.empty((K, H, W), dtype=torch.int32, device=dev)
    bad = torch.empty(K, dtype=torch.int32, device=dev)
    rgba = torch.empty((K, H, W, 4), dtype=torch.uint8, device=dev)
    index = torch.empty((K, H, W), dtype=torch.int64, device=dev)
    depth = torch.empty((K, H, W), dtype=torch.int32, device=dev)
    splat = lambda: _hip.render_splat(pts, offsets, cam, vt, (H, W), keys, count, bad)                  # noqa: E731
    nolook = lambda: _hip.render_splat(pts, offsets, cam, vt, (H, W), keys, count, bad, look=False)     # noqa: E731
    always = lambda: _hip.render_splat(pts, offsets, cam, vt, (H, W), keys, count, bad, look=True)      # noqa: E731
    nocount = lambda: _hip.render_splat(pts, offsets, cam, vt, (H, W), keys, None, bad)                 # noqa: E731
    resolve = lambda: _hip.render_resolve(keys, (H, W), offsets, vt, rgb16, _hip.SN_RENDER_RGB16, (255,) * 4, 0.0, rgba, index, depth)   # noqa: E731
    shaded = lambda: _hip.render_resolve(keys, (H, W), offsets, vt, rgb16, _hip.SN_RENDER_RGB16, (255,) * 4, 4.0, rgba, index, depth)    # noqa: E731
    nolook()
    first = keys.clone()
    for fn in (always, nocount, splat):
        keys.fill_(5)
        fn()
        assert torch.equal(keys, first) and int(bad.sum()) == 0
    off = offsets.cpu().tolist()
    for k in range(min(K, check_views)):
        lo, hi = off[view_tile[k]], off[view_tile[k] + 1]
        assert torch.equal(keys[k].view(-1), torch_keys(pts[lo:hi], cams[k], H, W)), f"{name}: view {k} differs from torch"
    fore = int((keys != -1).sum())
    accepted = int(count.sum())
    res = {"views": K, "point_size": int(cams[0][15]), "kind": "perspective" if cams[0][12] == 1.0 else "orthographic",
           "rows_drawn": accepted, "foreground_pixels": fore, "rows_per_foreground_pixel": round(accepted / max(fore, 1), 1),
           "splat": both_ways(splat, args.iters), "splat_no_look": both_ways(nolook, args.iters),
           "splat_look_always": both_ways(always, args.iters), "splat_without_count": both_ways(nocount, args.iters),
           "resolve": both_ways(resolve, args.iters), "resolve_shaded": both_ways(shaded, args.iters)}
    res["look_gain"] = round(res["splat_no_look"]["graph_replay_us"] / res["splat_look_always"]["graph_replay_us"], 3)
    res["against_the_mark"] = verdict(res["splat"], yard)
    res["per_view_over_yardstick"] = round(res["against_the_mark"]["over_yardstick"] / K, 3)
    print(name, json.dumps(res), flush=True)
    return res


def yardstick(pts, args):
    """sn_crop_count over the rows with one box region: 24 B per point read once"""
    dev = pts.device
    n = int(pts.shape[0])
    box = torch.tensor([[-1e9, -1e9, 1e9, 1e9]], dtype=torch.float64, device=dev)
    kinds = torch.tensor([_hip.SN_CROP_BOX], dtype=torch.int32, device=dev)
    ws = torch.empty(_hip.crops_ws_bytes(n, 1) // 8, dtype=torch.int64, device=dev)
    offsets = torch.empty(2, dtype=torch.int64, device=dev)
    fn = lambda: _hip.crop_count(pts, box, kinds, ws, offsets)   # noqa: E731
    fn()
    assert int(offsets[1]) == n
    res = both_ways(fn, args.iters)
    res["hbm_share_of_peak"] = round(n * 24 / (res["graph_replay_us"] * 1e-6) / HBM_PEAK, 3)
    return res


def scan_cases(args):
    dev = torch.device("cuda:0")
    xyz, lab, _ = synthetic_scan(args.points)
    n = len(xyz)
    print(f"scan: {n} points", flush=True)
    pts = torch.from_numpy(xyz).to(dev)
    offsets = torch.tensor([0, n], dtype=torch.int64, device=dev)
    rgb16 = sna.class_colors(torch.from_numpy(lab).to(dev), sna.default_class_table(), las=True).rgb
    lo, hi = xyz.min(axis=0), xyz.max(axis=0)
    S = args.size
    yard = yardstick(pts, args)
    res = {"points": n, "size": [S, S], "yardstick_crop_count_one_box": yard}
    centre = (lo + hi) / 2
    eye = centre + np.array([-0.9, -0.7, 0.5]) * np.linalg.norm(hi - lo)
    far = 3.0 * float(np.linalg.norm(hi - lo))
    for s in (1, 3):
        top = sna.ortho_camera(lo, hi, "top", S, S, point_size=s)
        three = [sna.ortho_camera(lo, hi, v, S, S, point_size=s) for v in ("top", "front", "side")]
        res[f"top_s{s}"] = case(f"scan top s={s}", pts, offsets, rgb16, [top], [0], args, yard)
        res[f"three_views_s{s}"] = case(f"scan 3 views s={s}", pts, offsets, rgb16, three, [0, 0, 0], args, yard, check_views=3 if s == 1 else 1)
    persp = sna.perspective_camera(eye, centre, (0, 0, 1), 40.0, S, S, 1.0, far)
    res["perspective_s1"] = case("scan perspective s=1", pts, offsets, rgb16, [persp], [0], args, yard)
    # the same image without this library: torch on the device, matplotlib on the host
    top = sna.ortho_camera(lo, hi, "top", S, S)
    t_torch = timed(lambda: torch_keys(pts, top, S, S), max(2, args.iters // 4))
    m = min(args.host_points, n)
    d2h, plot = host_scatter(pts, rgb16, m)
    mine = res["top_s1"]["splat"]["graph_replay_us"] + res["top_s1"]["resolve"]["graph_replay_us"]
    res["baselines"] = {"torch_project_scatter_reduce_amin_us": round(t_torch * 1e3, 1),
                        "torch_over_splat_replay": round(t_torch * 1e3 / res["top_s1"]["splat"]["graph_replay_us"], 2),
                        "host_points_timed": m, "host_copy_down_ms": round(d2h * 1e3, 2), "host_matplotlib_scatter_ms": round(plot * 1e3, 1),
                        "host_scaled_ms": round((d2h + plot) * 1e3 * n / m, 1),
                        "host_note": "the copy down and one matplotlib 3-D scatter saved as a PNG, timed on host_points_timed points and scaled linearly to the scan",
                        "host_over_splat_plus_resolve_replay": round((d2h + plot) * n / m * 1e6 / mine, 1)}
    png_t0 = time.perf_counter()
    data = sna.png_bytes(torch.empty((S, S, 4), dtype=torch.uint8, device=dev).fill_(200))
    res["png_bytes_of_a_flat_image_ms"] = round((time.perf_counter() - png_t0) * 1e3, 2)
    res["png_bytes_len"] = len(data)
    print(json.dumps(res["baselines"]), flush=True)
    return res


def batch_cases(args):
    dev = torch.device("cuda:0")
    tiles, labels = zip(*[synthetic_tile(t, args.tile_points) for t in range(args.batch)])
    sizes = [len(t) for t in tiles]
    pts = torch.from_numpy(np.concatenate(tiles)).to(dev)
    lab = torch.from_numpy(np.concatenate(labels)).to(dev)
    offsets = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int64, device=dev)
    B = len(sizes)
    print(f"batch: {int(pts.shape[0])} points in {B} tiles", flush=True)
    rgb16 = sna.class_colors(lab, sna.default_class_table(), offsets=offsets, las=True).rgb
    S = args.size
    yard = yardstick(pts, args)
    res = {"points": int(pts.shape[0]), "tiles": B, "size": [S, S], "yardstick_crop_count_one_box": yard}
    for s in (1, 3):
        cams = [sna.ortho_camera(t.min(axis=0), t.max(axis=0), "top", S, S, point_size=s) for t in tiles]
        res[f"top_of_every_tile_s{s}"] = case(f"batch top s={s}", pts, offsets, rgb16, cams, list(range(B)), args, yard)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="render_bench.json")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--points", type=int, default=10_000_000)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--tile-points", type=int, default=100_000)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--host-points", type=int, default=100_000, help="points the host baseline runs (scaled to the scan)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("render_bench needs a HIP device (there is no CPU path)")
    res = {"device": torch.cuda.get_device_name(0), "chunk_points": _hip.render_chunk_points(), "hbm_peak_bytes_per_s": HBM_PEAK,
           "allowance": ALLOWANCE, "iters": args.iters}
    res["scan"] = scan_cases(args)
    res["batch_c2"] = batch_cases(args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
