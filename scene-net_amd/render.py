"""Point clouds to images on the device: a z-buffer point rasteriser (sn_render_splat / sn_render_resolve,
csrc/render.hip).

The reference looks at its results through a viewer window or a matplotlib 3-D scatter on the host (visualize_ply,
plot_voxelgrid(plot=True), visualize_pred_vs_gt, plot_centroids, visualize_batch; three times per logged batch in
LitSceneNet.on_validation_batch_end).  Here the coloured rows that voxel_cloud, class_colors and shape_colors leave in HBM
become PNG images without the points leaving the device:

    views = sna.render_scan(xyz, classes=classes, views=('top', 'front', 'side'), size=(1024, 1024), edl=4.0)
    sna.write_png("top.png", views.rgba[0])
    row = views.index[0, y, x]                                  # the pick buffer: which scan point is under this pixel
    sna.render_voxelgrid(pred, 'ranges', desc=grids.desc)       # K16's rows as images, one voxel one splat
    sna.render_pred_vs_gt(pred, gt, tau=0.5)                    # the reference's (4 pred + gt) / 5 under the 'ranges' colours

Definition (normative, include/scenenet_hip.h): a row is projected by a 3 x 4 matrix in fp64, each operation rounded once;
the accepted row's key (depth quantum << 32 | row in tile) goes into the s x s pixels around it by unsigned 64-bit minimum:
nearest depth wins, the lowest row among equal quanta.  Image x grows to the right and y DOWNWARDS; a smaller depth is
nearer.  There is no hole filling, no anti-aliasing and no perspective-scaled splat; there is no interactive viewer.
There is no CPU path: CPU tensors raise HipLibraryError.
"""
from __future__ import annotations

import math
import struct
import zlib
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _hip
from ._hip import SN_RENDER_DEPTH, SN_RENDER_MAX_SPLAT, SN_RENDER_MAX_VIEWS, SN_RENDER_RGB16, HipLibraryError

# (right, up) of the named views; the camera looks along -(right x up).  'top': from above, north up; 'front': from the
# south, looking north; 'side': from the east, looking west.
_NAMED = {
    "top": ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0)),
    "front": ((1.0, 0.0, 0.0), (0.0, 0.0, 1.0)),
    "side": ((0.0, 1.0, 0.0), (0.0, 0.0, 1.0)),
}


def _view_axes(view) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(right, up, forward) unit vectors of a named view or of (azimuth_deg, elevation_deg): the camera sits at that
    azimuth (from +x towards +y) and elevation above the horizon and looks at the box's centre."""
    if isinstance(view, str):
        if view not in _NAMED:
            raise ValueError(f"view must be one of {sorted(_NAMED)} or (azimuth_deg, elevation_deg); got {view!r}")
        right, up = (np.array(v) for v in _NAMED[view])
    else:
        az, el = (math.radians(float(v)) for v in view)
        ca, sa, ce, se = math.cos(az), math.sin(az), math.cos(el), math.sin(el)
        right = np.array([-sa, ca, 0.0])
        up = np.array([-se * ca, -se * sa, ce])
    return right, up, -np.cross(right, up)


def _point_size(point_size) -> float:
    s = int(point_size)
    if s != point_size or not 1 <= s <= SN_RENDER_MAX_SPLAT:
        raise ValueError(f"point_size must be an integer in 1..{SN_RENDER_MAX_SPLAT} (got {point_size})")
    return float(s)


def ortho_camera(lo, hi, view="top", width: int = 1024, height: int = 1024, margin: float = 0.02,
                 point_size: int = 1) -> np.ndarray:
    """The [16] fp64 camera row (numpy, host) of an orthographic view that fits the box lo..hi into a width x height image
    at ONE scale for both axes, `margin` of each side left free.  near / far come from the box's extent along the view
    direction, widened by a thousandth of it and by 1e-7 of the coordinates' magnitude so that the box's own corners pass
    near <= d < far whatever the rounding."""
    lo, hi = np.asarray(lo, dtype=np.float64).reshape(3), np.asarray(hi, dtype=np.float64).reshape(3)
    if not (np.all(np.isfinite(lo)) and np.all(np.isfinite(hi)) and np.all(lo <= hi)):
        raise ValueError(f"the box must be finite with lo <= hi (got {lo}, {hi})")
    if not 0.0 <= margin < 0.5:
        raise ValueError(f"margin must be in [0, 0.5) (got {margin})")
    right, up, fwd = _view_axes(view)
    corners = np.array([[(lo, hi)[i][0], (lo, hi)[j][1], (lo, hi)[k][2]] for i in (0, 1) for j in (0, 1) for k in (0, 1)])
    centre = (lo + hi) / 2.0
    rel = corners - centre
    u, v, d = rel @ right, rel @ up, rel @ fwd
    eu, ev = u.max() - u.min(), v.max() - v.min()
    free = 1.0 - 2.0 * margin
    scales = [free * n / e for n, e in ((width, eu), (height, ev)) if e > 0.0]
    scale = min(scales) if scales else 1.0
    cam = np.zeros(16, dtype=np.float64)
    cam[0:3] = scale * right
    cam[3] = width / 2.0 - scale * (centre @ right + (u.max() + u.min()) / 2.0)
    cam[4:7] = -scale * up
    cam[7] = height / 2.0 + scale * (centre @ up + (v.max() + v.min()) / 2.0)
    cam[8:11] = fwd
    cam[11] = -(centre @ fwd)
    span = d.max() - d.min()
    pad = 1e-3 * span + 1e-7 * float(np.abs(corners).max()) + 1e-12
    cam[12] = 0.0
    cam[13] = d.min() - pad
    cam[14] = d.max() + pad
    cam[15] = _point_size(point_size)
    return cam


def perspective_camera(eye, target, up, fov_y_deg: float, width: int, height: int, near: float, far: float,
                       point_size: int = 1) -> np.ndarray:
    """The [16] fp64 camera row (numpy, host) of a pinhole at `eye` looking at `target`: the rows of A are K [R | t], so
    px = c0 / c2, py = c1 / c2 and the depth is the distance along the view direction.  The target projects to the image
    centre (width / 2, height / 2)."""
    eye, target, up = (np.asarray(v, dtype=np.float64).reshape(3) for v in (eye, target, up))
    fwd = target - eye
    n = np.linalg.norm(fwd)
    if not n > 0.0:
        raise ValueError("eye and target coincide")
    fwd = fwd / n
    right = np.cross(fwd, up)
    n = np.linalg.norm(right)
    if not n > 0.0:
        raise ValueError("up is parallel to the view direction")
    right = right / n
    down = -np.cross(right, fwd)
    if not 0.0 < fov_y_deg < 180.0:
        raise ValueError(f"fov_y_deg must be in (0, 180) (got {fov_y_deg})")
    if not 0.0 < near < far:
        raise ValueError(f"a perspective camera needs 0 < near < far (got {near}, {far})")
    f = (height / 2.0) / math.tan(math.radians(fov_y_deg) / 2.0)
    R = np.stack([right, down, fwd])
    Kmat = np.array([[f, 0.0, width / 2.0], [0.0, f, height / 2.0], [0.0, 0.0, 1.0]])
    A = Kmat @ np.concatenate([R, (-R @ eye)[:, None]], axis=1)
    cam = np.zeros(16, dtype=np.float64)
    cam[:12] = A.reshape(-1)
    cam[12], cam[13], cam[14], cam[15] = 1.0, float(near), float(far), _point_size(point_size)
    return cam


@dataclass
class RenderedViews:
    """What one render_points call leaves on the device: K images of H x W pixels.
      rgba      [K,H,W,4] uint8
      index     [K,H,W] int64: the winner's row in the packed batch, -1 for background (with `into=`: a row of the layer
                `layer` names)
      depth_q   [K,H,W] int32 holding the u32 depth quanta (background 2^32 - 1, read as -1)
      count     [K,H,W] int32 holding the u32 number of accepted rows whose centre fell on the pixel | None
      keys      [K,H,W] int64 holding the u64 keys (depth quantum << 32 | row in tile; background all ones)
      bad_views [K] int32: 1 for a camera row that shows nothing
      layer     [K,H,W] int32 | None: with `into=`, which call's row won the pixel (0 the first)
      cameras   [K,16] f64 and view_tile [K] int32 as they were used"""
    rgba: torch.Tensor
    index: torch.Tensor
    depth_q: torch.Tensor
    count: Optional[torch.Tensor]
    keys: torch.Tensor
    bad_views: torch.Tensor
    cameras: torch.Tensor
    view_tile: torch.Tensor
    layer: Optional[torch.Tensor] = None
    layers: int = 1

    @property
    def K(self) -> int:
        return int(self.rgba.shape[0])

    @property
    def size(self) -> Tuple[int, int]:
        return int(self.rgba.shape[1]), int(self.rgba.shape[2])

    def check(self) -> None:
        """Raises ValueError when a camera row showed nothing.  Synchronises."""
        bad = [k for k, v in enumerate(self.bad_views.cpu().tolist()) if v]
        if bad:
            raise ValueError(f"views {bad} have a camera row that shows nothing (unknown kind, point size outside "
                             f"1..{SN_RENDER_MAX_SPLAT}, near >= far, or perspective with near <= 0)")

    def png(self, k: int = 0) -> bytes:
        return png_bytes(self.rgba[k])


def _device_rows(t, name: str, dtype, cols: int) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise HipLibraryError(f"{name} must live on a HIP device; there is no CPU path")
    if t.dim() != 2 or t.shape[1] != cols:
        raise ValueError(f"{name} must be [total, {cols}] (got {tuple(t.shape)})")
    return t.to(dtype).contiguous() if dtype is not None else t.contiguous()


def _cameras(cameras, dev) -> torch.Tensor:
    if isinstance(cameras, torch.Tensor):
        if not cameras.is_cuda:
            raise HipLibraryError("a cameras tensor must live on a HIP device (or pass numpy rows); there is no CPU path")
        cam = cameras.to(torch.float64)
    else:
        rows = np.asarray(cameras, dtype=np.float64)
        cam = torch.from_numpy(np.ascontiguousarray(rows)).to(dev)
    cam = cam.reshape(-1, 16).contiguous()
    if not 1 <= cam.shape[0] <= SN_RENDER_MAX_VIEWS:
        raise ValueError(f"1 .. {SN_RENDER_MAX_VIEWS} cameras are served (got {cam.shape[0]})")
    return cam


def render_points(xyz, rgb16=None, offsets: Optional[torch.Tensor] = None, cameras=None, view_tile=None,
                  size: Sequence[int] = (1024, 1024), edl: float = 0.0,
                  background: Sequence[int] = (255, 255, 255, 255), into: Optional[RenderedViews] = None,
                  want_count: bool = True) -> RenderedViews:
    """K images of a CSR batch of point clouds in two launches (three with the clearing one); nothing is read back.
      xyz        [total,3] f64 on the device
      rgb16      [total,3] uint16 (what class_colors(las=True), shape_colors and voxel_cloud(las=True) give): a pixel takes
                 the high byte of each channel.  None: the depth as a grey, near white and far black
      offsets    [B+1] int64 on the device; None: one tile, the whole array
      cameras    [K,16] rows from ortho_camera / perspective_camera (numpy, or a device tensor)
      view_tile  [K]: the tile view k shows; None: view k shows tile k when K == B, every view tile 0 when B == 1
      size       (H, W)
      edl        >= 0: depth-difference shading (header); 0 off
      want_count False: no `count` image (one atomic per row and view less)
      into       an earlier result with the same size and number of views: the new rows are composited onto its keys with
                 SN_RENDER_ACCUMULATE (cameras and view_tile default to its own; another point size is the usual reason to
                 give them) and the pixels a new row won take the new layer's colour, index and shade; the others keep
                 what they had (an equal key, the same depth quantum and row number, leaves the pixel to the earlier layer).
                 `layer` tells which call won a pixel.  `into` itself is not modified; one rendered with want_count=False
                 needs want_count=False here too."""
    pts = _device_rows(xyz, "xyz", torch.float64, 3)
    dev, total = pts.device, int(pts.shape[0])
    if total == 0:
        raise ValueError("render_points needs at least one point")
    if rgb16 is not None:
        if isinstance(rgb16, torch.Tensor) and rgb16.dtype not in (torch.uint16, torch.int16):
            raise HipLibraryError(f"rgb16 must be uint16 (got {rgb16.dtype})")
        rgb16 = _device_rows(rgb16, "rgb16", None, 3)
        if int(rgb16.shape[0]) != total:
            raise ValueError("xyz and rgb16 disagree in length")
    if offsets is None:
        offsets = torch.tensor([0, total], dtype=torch.int64, device=dev)
    elif not isinstance(offsets, torch.Tensor) or not offsets.is_cuda:
        raise HipLibraryError("offsets must live on a HIP device; there is no CPU path")
    B = int(offsets.numel()) - 1
    if cameras is None:
        if into is None:
            raise ValueError("render_points needs cameras")
        cameras = into.cameras
    cam = _cameras(cameras, dev)
    K = int(cam.shape[0])
    if view_tile is None:
        if into is not None:
            view_tile = into.view_tile
        elif K == B:
            view_tile = torch.arange(K, dtype=torch.int32, device=dev)
        elif B == 1:
            view_tile = torch.zeros(K, dtype=torch.int32, device=dev)
        else:
            raise ValueError(f"view_tile is needed for {K} views of {B} tiles")
    if not isinstance(view_tile, torch.Tensor):
        view_tile = torch.tensor([int(v) for v in view_tile], dtype=torch.int32)
    view_tile = view_tile.to(device=dev, dtype=torch.int32).contiguous()
    if int(view_tile.numel()) != K:
        raise ValueError(f"view_tile must hold one tile per camera ({K}; got {int(view_tile.numel())})")
    H, W = (int(v) for v in size)
    mode = SN_RENDER_DEPTH if rgb16 is None else SN_RENDER_RGB16
    rgba = torch.empty((K, H, W, 4), dtype=torch.uint8, device=dev)
    index = torch.empty((K, H, W), dtype=torch.int64, device=dev)
    depth_q = torch.empty((K, H, W), dtype=torch.int32, device=dev)
    if into is None:
        keys = torch.empty((K, H, W), dtype=torch.int64, device=dev)
        count = torch.empty((K, H, W), dtype=torch.int32, device=dev) if want_count else None
        bad = torch.empty((K,), dtype=torch.int32, device=dev)
        _hip.render_splat(pts, offsets, cam, view_tile, (H, W), keys, count, bad)
        _hip.render_resolve(keys, (H, W), offsets, view_tile, rgb16, mode, background, edl, rgba, index, depth_q)
        return RenderedViews(rgba, index, depth_q, count, keys, bad, cam, view_tile)
    if tuple(into.keys.shape) != (K, H, W):
        raise ValueError(f"`into` holds images of shape {tuple(into.keys.shape)}, this call {(K, H, W)}")
    if want_count and into.count is None:
        raise ValueError("`into` was rendered without a count image: pass want_count=False")
    keys, bad = into.keys.clone(), into.bad_views.clone()
    count = into.count.clone() if want_count else None
    _hip.render_splat(pts, offsets, cam, view_tile, (H, W), keys, count, bad, accumulate=True)
    # A key's low word is a row of ITS call's batch, so this resolve, made with the new layer's offsets and rgb16, is right
    # only where a new row won; elsewhere it reads an old key against the new batch (kept inside it by the kernel's own
    # "row below the tile's size" test) and the masks below throw that pixel away.  A new row wins where it changed the key:
    # an equal key (same depth quantum, same row number in its tile) leaves the pixel to the earlier layer.
    _hip.render_resolve(keys, (H, W), offsets, view_tile, rgb16, mode, background, edl, rgba, index, depth_q)
    won = keys != into.keys
    before = into.layer if into.layer is not None else torch.zeros((K, H, W), dtype=torch.int32, device=dev)
    return RenderedViews(torch.where(won[..., None], rgba, into.rgba), torch.where(won, index, into.index),
                         torch.where(won, depth_q, into.depth_q), count, keys, bad, cam, view_tile,
                         torch.where(won, torch.full_like(before, into.layers), before), into.layers + 1)


def default_class_table(rows: int = 256) -> np.ndarray:
    """[rows,3] f64 in 0..1: hues a golden angle apart at two brightnesses -- a fixed table, so the same classes get the same
    colours in every image.  Row k colours a tile's k-th smallest class (class_colors)."""
    k = np.arange(int(rows), dtype=np.float64)
    h = (k * 0.6180339887498949) % 1.0
    v = np.where(k.astype(np.int64) % 2 == 0, 0.9, 0.6)
    i = np.floor(h * 6.0)
    f = h * 6.0 - i
    p, q, t = v * 0.25, v * (1.0 - 0.75 * f), v * (1.0 - 0.75 * (1.0 - f))
    i = i.astype(np.int64) % 6
    r = np.choose(i, [v, q, p, p, t, v])
    g = np.choose(i, [t, v, v, q, p, p])
    b = np.choose(i, [p, p, t, v, v, q])
    return np.stack([r, g, b], axis=1)


def _boxes(pts: torch.Tensor, offsets: torch.Tensor) -> np.ndarray:
    """[B,6] (lo, hi) of every tile, reduced on the device (sn_voxel_bbox); one copy of 48 B per tile.  Synchronises."""
    return _hip.voxel_bbox(pts, offsets).cpu().numpy()


def render_scan(xyz, classes=None, rgb16=None, views: Sequence = ("top", "front", "side"),
                size: Sequence[int] = (1024, 1024), class_color=None, point_size: int = 1, margin: float = 0.02,
                edl: float = 0.0, background: Sequence[int] = (255, 255, 255, 255)) -> RenderedViews:
    """One scan, len(views) images, one call: the box comes from the device (sn_voxel_bbox, 48 bytes read back), the
    cameras are fitted to it on the host, and the colours are `rgb16`, or sna.class_colors(classes, class_color, las=True)
    (class_color None: default_class_table), or the depth as a grey when neither is given."""
    pts = _device_rows(xyz, "xyz", torch.float64, 3)
    if int(pts.shape[0]) == 0:
        raise ValueError("render_scan needs at least one point")
    if classes is not None:
        if rgb16 is not None:
            raise ValueError("classes and rgb16 are mutually exclusive")
        from .voxel_classes import class_colors
        rgb16 = class_colors(classes, default_class_table() if class_color is None else class_color, las=True).rgb
    H, W = (int(v) for v in size)
    offsets = torch.tensor([0, int(pts.shape[0])], dtype=torch.int64, device=pts.device)
    box = _boxes(pts, offsets)[0]
    cams = np.stack([ortho_camera(box[:3], box[3:], v, W, H, margin, point_size) for v in views])
    return render_points(pts, rgb16, offsets, cams, None, (H, W), edl, background)


def _voxel_point_size(cam: np.ndarray, voxel) -> int:
    """The splat that covers one voxel of edge lengths `voxel` at an orthographic camera's scale: ceil(scale * the largest
    edge), kept in 1 .. SN_RENDER_MAX_SPLAT."""
    scale = float(np.linalg.norm(cam[0:3]))
    return int(min(max(math.ceil(scale * float(np.max(voxel)) - 1e-9), 1), SN_RENDER_MAX_SPLAT))


def _grid_cameras(shape: Sequence[int], desc: Optional[np.ndarray], views: Sequence, size: Sequence[int],
                  margin: float = 0.02) -> np.ndarray:
    """The [B * len(views), 16] cameras render_voxelgrid uses for B grids of shape (nz, nx, ny): grid b's views in order,
    each fitted to the grid's box with the point size of one voxel.  desc [B, desc_len] (host): the box is its lo, hi and a
    voxel's edges the first step of its three edge tables -- right for a size-mode descriptor too, whose box is the tile's
    own and whose tables are padded.  None: the index box -0.5 .. n - 0.5, voxels of edge 1."""
    nz, nx, ny = (int(v) for v in shape)
    n = np.array([nx, ny, nz], dtype=np.float64)
    H, W = (int(v) for v in size)
    B = 1 if desc is None else len(desc)
    rows = []
    for b in range(B):
        if desc is None:
            lo, hi, voxel = -0.5 * np.ones(3), n - 0.5, np.ones(3)
        else:
            lo, hi = desc[b, :3], desc[b, 3:6]
            first = (6, 6 + nx + 1, 6 + nx + 1 + ny + 1)
            voxel = np.array([desc[b, f + 1] - desc[b, f] for f in first])
        for v in views:
            cam = ortho_camera(lo, hi, v, W, H, margin, 1)
            cam[15] = float(_voxel_point_size(cam, voxel))
            rows.append(cam)
    return np.stack(rows)


def render_voxelgrid(grids: torch.Tensor, color_mode: str = "density", views: Sequence = ("top", "front", "side"),
                     desc: Optional[torch.Tensor] = None, size: Sequence[int] = (512, 512), r: int = 10, color_ranges=None,
                     margin: float = 0.02, edl: float = 0.0,
                     background: Sequence[int] = (255, 255, 255, 255)) -> Optional[RenderedViews]:
    """plot_voxelgrid as images: K16's voxel_cloud(grids, color_mode, las=True) rows through render_points, len(views) images
    per grid (grid b's are b * len(views) ...), each voxel a splat that covers it at the camera's scale.  grids [B,nz,nx,ny]
    or [B,1,nz,nx,ny] on the device.  With `desc` the images are in scan coordinates (the descriptor is read back: a few
    hundred bytes per grid).  Returns None when no grid has a voxel to show (plot_voxelgrid returns None there)."""
    from .voxel_cloud import voxel_cloud
    cloud = voxel_cloud(grids, color_mode, r, color_ranges, desc=desc, las=True)
    if int(cloud.xyz.shape[0]) == 0:
        return None
    shape = tuple(grids.shape[-3:])
    B = cloud.B
    boxes = None if desc is None else desc.cpu().numpy()
    cams = _grid_cameras(shape, boxes, views, size, margin)
    if boxes is None:
        cams = np.tile(cams, (B, 1))
    view_tile = np.repeat(np.arange(B), len(views))
    return render_points(cloud.xyz, cloud.rgb, cloud.offsets, cams, view_tile, size, edl, background)


def render_pred_vs_gt(pred: torch.Tensor, gt: torch.Tensor, tau: float, **kwargs) -> Optional[RenderedViews]:
    """visualize_pred_vs_gt (utils/voxelization.py:364-381) as images: (4 * prob_to_label(pred, tau) + gt) / 5 under the
    'ranges' colours -- 1 a true positive, 0.8 a false positive, 0.2 a miss.  pred and gt [B,nz,nx,ny] or [B,1,nz,nx,ny]
    on the device; kwargs go to render_voxelgrid."""
    for name, t in (("pred", pred), ("gt", gt)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise HipLibraryError(f"{name} must live on a HIP device; there is no CPU path")
    from .voxelization import prob_to_label
    common = (4 * prob_to_label(pred.to(torch.float64), tau) + 1 * gt.to(torch.float64)) / 5
    return render_voxelgrid(common, "ranges", **kwargs)


def _chunk(tag: bytes, data: bytes) -> bytes:
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)


def png_bytes(rgba: Union[torch.Tensor, np.ndarray], level: int = 6) -> bytes:
    """A PNG file of one [H,W,4] uint8 image: 8-bit RGBA, every scanline with filter 0, one IDAT chunk; zlib and struct
    only.  A device tensor costs one copy of H * W * 4 bytes to the host."""
    a = rgba.detach().cpu().numpy() if isinstance(rgba, torch.Tensor) else np.asarray(rgba)
    if a.ndim != 3 or a.shape[2] != 4 or a.dtype != np.uint8 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f"png_bytes takes one [H, W, 4] uint8 image (got {a.dtype} {a.shape})")
    H, W = int(a.shape[0]), int(a.shape[1])
    lines = np.zeros((H, 1 + 4 * W), dtype=np.uint8)
    lines[:, 1:] = a.reshape(H, 4 * W)
    return (b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 6, 0, 0, 0)) +
            _chunk(b"IDAT", zlib.compress(lines.tobytes(), level)) + _chunk(b"IEND", b""))


def write_png(path: str, rgba: Union[torch.Tensor, np.ndarray]) -> int:
    """png_bytes to a file; returns the bytes written."""
    data = png_bytes(rgba)
    with open(path, "wb") as f:
        f.write(data)
    return len(data)
