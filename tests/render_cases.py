"""K23's oracle and cases: the rule of include/scenenet_hip.h restated in numpy operation for operation (splat_oracle,
resolve_oracle) and the inputs the host and GPU tests share.  Every builder asserts on the CPU that its case exercises what
it is for, so a test cannot pass vacuously.  Seeds are fixed; oracles are computed once per process (functools.lru_cache)
and must be left unchanged by their users."""
import functools
import struct
import zlib
from typing import NamedTuple

import numpy as np

from scene_net_amd import _hip
from scene_net_amd.render import ortho_camera

BACKGROUND = np.uint64(0xFFFFFFFFFFFFFFFF)
MAX_Q = np.uint64(0xFFFFFFFF)
TWO32 = 4294967296.0
LIMIT = 1073741824.0          # 2^30
RGB16, DEPTH = _hip.SN_RENDER_RGB16, _hip.SN_RENDER_DEPTH
EDLS = (0.0, 0.5, 1e6)
WHITE = (255, 255, 255, 255)


class Case(NamedTuple):
    pts: np.ndarray           # [total, 3] f64
    offsets: np.ndarray       # [B + 1] i64
    cam: np.ndarray           # [K, 16] f64
    view_tile: np.ndarray     # [K] i32
    H: int
    W: int


# ------------------------------------------------------------------ the rule
def camera_ok(c) -> bool:
    kind, near, far, s = (float(v) for v in c[12:16])
    if not (kind == 0.0 or kind == 1.0):
        return False
    if not (1.0 <= s <= float(_hip.SN_RENDER_MAX_SPLAT)) or s != np.floor(s):
        return False
    if not near < far:
        return False
    with np.errstate(over="ignore"):
        if not np.float64(far) - np.float64(near) < np.inf:
            return False
    if kind == 1.0 and not near > 0.0:
        return False
    return True


def project(P, c):
    """(accepted [n] bool, dq [n] u64, ix [n] i64, iy [n] i64) of the rows P [n,3] under the camera row c, literally; dq,
    ix and iy are meaningful where accepted."""
    A = np.asarray(c[:12], dtype=np.float64).reshape(3, 4)
    near, far = np.float64(c[13]), np.float64(c[14])
    x, y, z = (np.ascontiguousarray(P[:, a], dtype=np.float64) for a in range(3))
    with np.errstate(all="ignore"):
        c0, c1, c2 = (((A[r, 0] * x + A[r, 1] * y) + A[r, 2] * z) + A[r, 3] for r in range(3))
        d = c2
        px, py = (c0 / d, c1 / d) if c[12] == 1.0 else (c0, c1)
        ok = (near <= d) & (d < far) & (np.abs(px) < LIMIT) & (np.abs(py) < LIMIT)
        q = np.floor(((d - near) / (far - near)) * TWO32)
    q = np.where(ok, q, 0.0)
    dq = np.minimum(q.astype(np.uint64), MAX_Q)
    ix = np.floor(np.where(ok, px, 0.0)).astype(np.int64)
    iy = np.floor(np.where(ok, py, 0.0)).astype(np.int64)
    return ok, dq, ix, iy


def splat_oracle(pts, offsets, cam, view_tile, H, W, keys=None, count=None, bad=None):
    """-> (keys [K,H,W] u64, count [K,H,W] u32, bad_views [K] i32).  keys / count / bad given: the accumulate form, onto
    copies of them."""
    K, B = len(cam), len(offsets) - 1
    keys = np.full((K, H, W), BACKGROUND, dtype=np.uint64) if keys is None else keys.copy()
    count = np.zeros((K, H, W), dtype=np.uint32) if count is None else count.copy()
    bad = np.zeros(K, dtype=np.int32) if bad is None else bad.copy()
    for k in range(K):
        c = cam[k]
        if not camera_ok(c):
            bad[k] = 1
            continue
        b = int(view_tile[k])
        if not 0 <= b < B:
            continue
        lo, hi = int(offsets[b]), int(offsets[b + 1])
        assert hi - lo < 2 ** 32 - 1
        if hi == lo:
            continue
        ok, dq, ix, iy = project(pts[lo:hi], c)
        j = np.flatnonzero(ok)
        key = (dq[j] << np.uint64(32)) | j.astype(np.uint64)
        ix, iy = ix[j], iy[j]
        s = int(c[15])
        for dy in range(-((s - 1) // 2), s // 2 + 1):
            for dx in range(-((s - 1) // 2), s // 2 + 1):
                X, Y = ix + dx, iy + dy
                m = (X >= 0) & (X < W) & (Y >= 0) & (Y < H)
                np.minimum.at(keys[k], (Y[m], X[m]), key[m])
        m = (ix >= 0) & (ix < W) & (iy >= 0) & (iy < H)
        np.add.at(count[k], (iy[m], ix[m]), np.uint32(1))
    return keys, count, bad


def resolve_oracle(keys, offsets, view_tile, rgb16, mode, background, edl):
    """-> (rgba [K,H,W,4] u8, index [K,H,W] i64, depth_q [K,H,W] u32)"""
    K, H, W = keys.shape
    B = len(offsets) - 1
    dq = (keys >> np.uint64(32)).astype(np.int64)
    j = (keys & MAX_Q).astype(np.int64)
    vt = np.asarray(view_tile, dtype=np.int64)
    tile_ok = (vt >= 0) & (vt < B)
    b = np.where(tile_ok, vt, 0)
    lo, n = offsets[b].astype(np.int64), (offsets[b + 1] - offsets[b]).astype(np.int64)
    fore = (keys != BACKGROUND) & tile_ok[:, None, None] & (j < n[:, None, None])
    index = np.where(fore, lo[:, None, None] + j, -1)
    depth_q = np.where(fore, dq, 2 ** 32 - 1).astype(np.uint32)
    if mode == DEPTH:
        grey = 255 - (dq >> 24)
        c = np.stack([grey, grey, grey], axis=-1)
    else:
        c = (rgb16[np.where(fore, index, 0)] >> 8).astype(np.int64)
    if edl != 0.0:
        o = np.zeros((K, H, W), dtype=np.int64)
        o[:, 1:, :] += np.maximum(0, dq[:, 1:, :] - dq[:, :-1, :])     # the neighbour above
        o[:, :-1, :] += np.maximum(0, dq[:, :-1, :] - dq[:, 1:, :])    # below
        o[:, :, 1:] += np.maximum(0, dq[:, :, 1:] - dq[:, :, :-1])     # left
        o[:, :, :-1] += np.maximum(0, dq[:, :, :-1] - dq[:, :, 1:])    # right
        shade = 1.0 / (1.0 + np.float64(edl) * (o.astype(np.float64) / TWO32))
        c = np.floor(c.astype(np.float64) * shade[..., None] + 0.5).astype(np.int64)
    rgba = np.empty((K, H, W, 4), dtype=np.uint8)
    rgba[..., :3] = c.astype(np.uint8)
    rgba[..., 3] = 255
    rgba[~fore] = np.array(background, dtype=np.uint8)
    return rgba, index, depth_q


# ------------------------------------------------------------------ helpers
def pixel_cam(s=1, near=0.0, far=1.0, kind=0.0, A=None):
    """px = x, py = y, d = z unless A [3,4] says otherwise"""
    c = np.zeros(16, dtype=np.float64)
    c[:12] = (np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], dtype=np.float64) if A is None else np.asarray(A)).reshape(-1)
    c[12], c[13], c[14], c[15] = kind, near, far, s
    return c


def one_tile(pts, cams, H, W, view_tile=None):
    pts = np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, 3)
    cams = np.ascontiguousarray(cams, dtype=np.float64).reshape(-1, 16)
    vt = np.zeros(len(cams), dtype=np.int32) if view_tile is None else np.asarray(view_tile, dtype=np.int32)
    return Case(pts, np.array([0, len(pts)], dtype=np.int64), cams, vt, H, W)


def colours(total, seed=230):
    """[total,3] u16 with both bytes of every word in use (the low byte must not show)"""
    return np.random.default_rng(seed).integers(0, 65536, (total, 3)).astype(np.uint16)


# ------------------------------------------------------------------ a PNG reader for what png_bytes writes
def read_chunks(data):
    assert data[:8] == b"\x89PNG\r\n\x1a\n", "the signature"
    pos, out = 8, []
    while pos < len(data):
        n, = struct.unpack(">I", data[pos:pos + 4])
        tag, body = data[pos + 4:pos + 8], data[pos + 8:pos + 8 + n]
        crc, = struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])
        assert crc == zlib.crc32(tag + body) & 0xFFFFFFFF, tag
        out.append((tag, body))
        pos += 12 + n
    assert pos == len(data)
    return out


def decode_png(data):
    chunks = read_chunks(data)
    assert [t for t, _ in chunks] == [b"IHDR", b"IDAT", b"IEND"] and chunks[2][1] == b""
    W, H, depth, colour, comp, filt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, colour, comp, filt, lace) == (8, 6, 0, 0, 0), "8-bit RGBA, deflate, adaptive filtering, not interlaced"
    raw = np.frombuffer(zlib.decompress(chunks[1][1]), dtype=np.uint8).reshape(H, 1 + 4 * W)
    assert (raw[:, 0] == 0).all(), "filter 0 on every scanline"
    return raw[:, 1:].reshape(H, W, 4)


# ------------------------------------------------------------------ the cases
def ties_case():
    rng = np.random.default_rng(231)
    H = W = 16
    xy = rng.random((300, 2)) * 16.0
    z = rng.integers(0, 8, 300) / 8.0                                  # eight depths: equal quanta are frequent
    base = np.concatenate([xy, z[:, None]], axis=1)
    dup = base[rng.integers(0, 300, 60)]                               # duplicate rows
    close = np.array([[3.25, 4.5, 0.5], [3.75, 4.25, 0.5 + 2.0 ** -40], [3.5, 4.75, 0.5 - 0.0]])   # one pixel, one quantum
    near_front = np.array([[3.1, 4.1, 0.5 + 2.0 ** -30]])              # the same pixel, four quanta behind
    P = np.concatenate([base, dup, close, near_front])
    P = P[rng.permutation(len(P))]
    case = one_tile(P, [pixel_cam(1), pixel_cam(3)], H, W)
    ok, dq, ix, iy = project(P, case.cam[0])
    assert ok.all()
    pix = iy * W + ix
    order = np.lexsort((dq, pix))
    p, q = pix[order], dq[order]
    first = np.r_[True, p[1:] != p[:-1]]                               # the nearest candidate of every pixel ...
    tied = ~first & np.r_[False, first[:-1]] & (q == np.r_[q[:1], q[:-1]])   # ... and a second one in the same quantum
    assert tied.sum() >= 10, "pixels whose two nearest candidates share a depth quantum"
    assert len(np.unique(P, axis=0)) < len(P), "duplicate rows"
    return case


def contraction_case():
    rng = np.random.default_rng(232)
    P = np.array([5.44e5, 4.634e6, 1.5e2]) + rng.random((20000, 3)) * np.array([30.0, 30.0, 60.0])
    cam = ortho_camera(P.min(axis=0), P.max(axis=0), (30.0, 20.0), 256, 256)
    case = one_tile(P, [cam], 256, 256)
    ok, dq, ix, iy = project(P, cam)
    assert ok.all() and ix.min() >= 0 and ix.max() < 256 and iy.min() >= 0 and iy.max() < 256
    # the same projection with the products and sums carried in extended precision and rounded once at the end: what a
    # contracted (fused multiply-add) build tends towards
    L = np.longdouble
    A = cam[:12].reshape(3, 4).astype(L)
    x, y, z = (P[:, a].astype(L) for a in range(3))
    e = [(A[r, 0] * x + A[r, 1] * y + A[r, 2] * z + A[r, 3]).astype(np.float64) for r in range(3)]
    edq = np.minimum(np.floor(((e[2] - cam[13]) / (cam[14] - cam[13])) * TWO32).astype(np.uint64), MAX_Q)
    differ = int((edq != dq).sum()) + int((np.floor(e[0]) != ix).sum()) + int((np.floor(e[1]) != iy).sum())
    assert differ >= 1, "no key tells the literal sequence from a contracted one"
    return case


EDGE_W, EDGE_H = 8, 6


def edges_case():
    W, H = EDGE_W, EDGE_H
    near, far = 1.0, 3.0
    up, down = (lambda v: np.nextafter(v, np.inf)), (lambda v: np.nextafter(v, -np.inf))
    nan, inf = np.nan, np.inf
    rows = [
        (2.0, 3.0, 2.0), (3.0, 0.0, 2.5),                              # 0, 1: exactly integral
        (-0.5, 1.5, 2.0), (-1e-300, 1.5, 2.0), (1.5, -0.5, 2.0), (1.5, -1e-300, 2.0),   # 2..5: floor, not truncation
        (W - 0.5, 2.5, 2.0), (float(W), 2.5, 2.0), (2.5, H - 0.5, 2.0), (2.5, float(H), 2.0),   # 6..9
        (4.5, 4.5, near), (5.5, 4.5, far),                             # 10 accepted, 11 rejected
        (4.5, 3.5, down(near)), (5.5, 3.5, up(near)), (6.5, 3.5, down(far)), (7.5, 3.5, up(far)),   # 12..15
        (nan, 1.0, 2.0), (1.0, nan, 2.0), (1.0, 1.0, nan), (inf, 1.0, 2.0), (1.0, -inf, 2.0), (1.0, 1.0, inf),   # 16..21
        (1.0, 1.0, -inf),                                              # 22
        (2.0 ** 30, 1.0, 2.0), (-2.0 ** 30, 1.0, 2.0), (1.0, 2.0 ** 30, 2.0), (down(2.0 ** 30), 1.0, 2.0),   # 23..26
        (1e300, 1.0, 2.0),                                             # 27
        (0.5, 0.5, 2.0 ** 53 - 1.0),                                   # 28: view 1's quotient rounds to 1.0
        (0.0, 0.0, 0.0), (1.0, 1.0, -1.0), (0.25, -0.25, 1.0), (0.0, 0.0, 0.5),   # 29..32: view 2, at / behind / before the eye
    ]
    P = np.array(rows, dtype=np.float64)
    f = 4.0
    persp = pixel_cam(1, 0.5, 10.0, 1.0, [[f, 0, W / 2, 0], [0, f, H / 2, 0], [0, 0, 1, 0]])
    cams = [pixel_cam(1, near, far), pixel_cam(2, -1.0, 2.0 ** 53), persp]
    case = one_tile(P, cams, H, W)
    ok, dq, ix, iy = project(P, cams[0])
    want = np.zeros(len(P), dtype=bool)
    want[[0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 13, 14, 26, 31]] = True   # (31: d == near again)
    assert np.array_equal(ok, want), np.flatnonzero(ok != want)
    assert ix[2] == -1 and ix[3] == -1 and iy[4] == -1 and iy[5] == -1 and ix[6] == W - 1 and ix[7] == W and iy[9] == H
    assert dq[10] == 0 and dq[13] == 0 and dq[14] == MAX_Q
    ok1, dq1, _, _ = project(P, cams[1])
    with np.errstate(all="ignore"):
        assert ((P[28, 2] + 1.0) / (2.0 ** 53 + 1.0)) * TWO32 == TWO32, "the quotient rounds to 1.0"
    assert ok1[28] and dq1[28] == MAX_Q, "and clamps to 2^32 - 1"
    ok2, _, ix2, iy2 = project(P, cams[2])
    assert not ok2[29] and not ok2[30] and ok2[31] and ok2[32] and (ix2[31], iy2[31]) == (5, 2) and (ix2[32], iy2[32]) == (4, 3)
    return case


SPLAT_SIZES = (1, 2, 3, 4, 9)


def splats_case():
    H, W = 7, 5
    rng = np.random.default_rng(233)
    X, Y = np.meshgrid(np.arange(-9, W + 10), np.arange(-9, H + 10))
    n = X.size
    P = np.stack([X.reshape(-1) + 0.5, Y.reshape(-1) + 0.25, (rng.permutation(n) + 0.5) / n], axis=1)
    case = one_tile(P, [pixel_cam(s) for s in SPLAT_SIZES], H, W)
    # even sizes are asymmetric: -(s-1)/2 .. +s/2
    for s, lo, hi in ((1, 0, 0), (2, 0, 1), (3, -1, 1), (4, -1, 2), (9, -4, 4)):
        assert (-((s - 1) // 2), s // 2) == (lo, hi)
        for ix, hit in ((-hi - 1, []), (-hi, [0]), (W - 1 - lo, [W - 1]), (W - lo, [])):
            one = one_tile([[ix + 0.5, 3.5, 0.5]], [pixel_cam(s)], H, W)
            keys, count, _ = splat_oracle(*one)
            cols = np.flatnonzero((keys[0] != BACKGROUND).any(axis=0)).tolist()
            assert cols == hit, (s, ix, cols, hit)
            assert count.sum() == (1 if 0 <= ix < W else 0)
    return case


SHAPE_SIZES = ((1, 1), (7, 5), (257, 129))
SHAPE_VIEWS = (1, 3, 64)


def shapes_case(H, W, K):
    c = _hip.render_chunk_points()
    sizes = [c - 1, 0, c, c + 1, 2 * c + 1, 37]                         # tile 1 is empty, tile 5 has no view
    rng = np.random.default_rng(234)
    P = rng.random((sum(sizes), 3))
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    view_tile = {1: [2], 3: [4, 3, 1], 64: [4 - (k % 5) for k in range(64)]}[K]      # descending; several views per tile
    assert all(a >= b for a, b in zip(view_tile[:4], view_tile[1:5])) and 5 not in view_tile
    if K > 1:
        assert 1 in view_tile, "a view of the empty tile"
    axes = ((0, 1, 2), (1, 2, 0), (2, 0, 1))
    cams = []
    for k in range(K):
        a = axes[k % 3]
        A = np.zeros((3, 4))
        A[0, a[0]], A[0, 3] = 1.2 * W, -0.1 * W                          # a tenth of the cloud hangs over every border
        A[1, a[1]], A[1, 3] = -1.2 * H, 1.1 * H                          # and this axis is flipped
        A[2, a[2]] = 1.0
        cams.append(pixel_cam(1 + k % 3, 0.0, 1.0 + k / 64.0, 0.0, A))
    case = Case(P, offsets, np.array(cams), np.array(view_tile, dtype=np.int32), H, W)
    keys, count, bad = oracle(("shapes", H, W, K), case)
    assert not bad.any()
    for k in range(K):
        assert (keys[k] != BACKGROUND).any() == (view_tile[k] != 1)
    return case


CONTENTION_N = 100000


def contention_case(order):
    n = CONTENTION_N
    i = np.arange(n, dtype=np.float64)
    z = {"decreasing": (n - i) / (n + 1.0), "increasing": (i + 1.0) / (n + 1.0), "equal": np.full(n, 0.5)}[order]
    P = np.stack([np.full(n, 1.5), np.full(n, 1.25), z], axis=1)
    case = one_tile(P, [pixel_cam(1)], 3, 3)
    ok, dq, ix, iy = project(P, case.cam[0])
    assert ok.all() and (ix == 1).all() and (iy == 1).all()
    step = np.diff(dq.astype(np.int64))
    assert {"decreasing": (step < 0).all(), "increasing": (step > 0).all(), "equal": (step == 0).all()}[order]
    keys, count, _ = oracle(("contention", order), case)
    winner = {"decreasing": n - 1, "increasing": 0, "equal": 0}[order]
    assert int(keys[0, 1, 1] & MAX_Q) == winner and count[0, 1, 1] == n and (keys != BACKGROUND).sum() == 1
    return case


def bad_cameras_case():
    rng = np.random.default_rng(235)
    H, W = 9, 11
    P = rng.random((500, 3)) * np.array([W, H, 1.0])
    P[:, 2] = 0.25 + 0.5 * P[:, 2]                                      # depths in 0.25 .. 0.75: inside every good camera
    nan, inf = np.nan, np.inf
    persp_A = [[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]]
    cams = [
        pixel_cam(1),                                                  # 0 good
        pixel_cam(1, kind=2.0), pixel_cam(1, kind=0.5), pixel_cam(1, kind=nan), pixel_cam(1, kind=-1.0),
        pixel_cam(0), pixel_cam(10), pixel_cam(2.5), pixel_cam(nan), pixel_cam(-3),
        pixel_cam(2),                                                  # 10 good (s = 2)
        pixel_cam(1, 0.5, 0.5), pixel_cam(1, 1.0, 0.0), pixel_cam(1, nan, 1.0), pixel_cam(1, 0.0, nan),
        pixel_cam(1, -1e308, 1e308), pixel_cam(1, -inf, inf),          # far - near is not finite
        pixel_cam(1, 0.0, 1.0, 1.0, persp_A), pixel_cam(1, -0.5, 1.0, 1.0, persp_A),   # perspective with near <= 0
        pixel_cam(1, 0.125, 1.0, 1.0, persp_A),                        # 19 good (perspective)
        pixel_cam(9),                                                  # 20 good
    ]
    good = [0, 10, 19, 20]
    case = one_tile(P, cams, H, W)
    keys, count, bad = oracle(("bad_cameras",), case)
    want = np.ones(len(cams), dtype=np.int32)
    want[good] = 0
    assert np.array_equal(bad, want)
    for k in range(len(cams)):
        assert (keys[k] != BACKGROUND).any() == (k in good) and (count[k] != 0).any() == (k in good)
    return case


# ------------------------------------------------------------------ shared, cached
_ORACLES = {}


def oracle(name, case):
    """splat_oracle of a named case, computed once"""
    if name not in _ORACLES:
        _ORACLES[name] = splat_oracle(*case)
    return _ORACLES[name]


@functools.lru_cache(maxsize=None)
def case(name):
    """name: a tuple -- ("ties",), ("contraction",), ("edges",), ("splats",), ("shapes", H, W, K), ("contention", order),
    ("bad_cameras",)"""
    return {"ties": ties_case, "contraction": contraction_case, "edges": edges_case, "splats": splats_case,
            "shapes": shapes_case, "contention": contention_case, "bad_cameras": bad_cameras_case}[name[0]](*name[1:])


CASE_NAMES = ([("ties",), ("contraction",), ("edges",), ("splats",), ("bad_cameras",)] +
              [("contention", o) for o in ("decreasing", "increasing", "equal")] +
              [("shapes", H, W, K) for (H, W) in SHAPE_SIZES for K in SHAPE_VIEWS])


def case_id(name):
    return "-".join(str(v) for v in name)
