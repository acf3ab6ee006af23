"""Scan crops (K9): the numpy oracle -- `scan[mask]` in exactly the reference's expressions (utils/pcd_processing.py:694-695,
:737, :836) -- and the case generators its host and GPU tests share.  Everything is compared exactly: integers as they
are, fp64 as int64 views."""
import functools
from fractions import Fraction

import numpy as np

DISC, BOX = 0, 1
ORIGIN = np.array([5.44e5, 4.634e6, 1.5e2])          # UTM-like, as the synthetic tiles
CENTRE = np.array([544000.0, 4634000.0])


def disc_mask(xyz, c_xy, radius):
    """pcd_processing.py:836 / :694: np.sum(np.power(xyz[:, :2] - c[:2], 2), axis=1) <= radius*radius"""
    with np.errstate(all="ignore"):
        return np.sum(np.power((xyz[:, :2] - np.asarray(c_xy, dtype=np.float64)), 2), axis=1) <= radius * radius


def box_mask(xyz, row):
    """pcd_processing.py:737: ((min1 <= a) & (a <= max2))[:, :2].all(axis=1), z disregarded"""
    lo, hi = np.asarray(row[:2], dtype=np.float64), np.asarray(row[2:4], dtype=np.float64)
    with np.errstate(all="ignore"):
        return ((lo <= xyz[:, :2]) & (xyz[:, :2] <= hi)).all(axis=1)


def region_mask(xyz, row, kind):
    if kind == DISC:
        return disc_mask(xyz, row[:2], float(row[2]))
    if kind == BOX:
        return box_mask(xyz, row)
    return np.zeros(xyz.shape[0], dtype=bool)      # any other kind: an empty region


def crop_oracle(pts, labels, regions, kinds=None):
    """(offsets [K+1] i64, rows [total,3], labels [total] | None, src [total] i64): tile k is scan[mask_k], in scan order"""
    K = regions.shape[0]
    kinds = np.zeros(K, dtype=np.int32) if kinds is None else kinds
    idx = [np.flatnonzero(region_mask(pts, regions[k], int(kinds[k]))) for k in range(K)]
    offsets = np.zeros(K + 1, dtype=np.int64)
    np.cumsum([len(i) for i in idx], out=offsets[1:])
    src = np.concatenate(idx).astype(np.int64) if K else np.zeros(0, dtype=np.int64)
    return offsets, pts[src], (None if labels is None else labels[src]), src


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


# ---- (a) random scans ------------------------------------------------------------------------------------------------
def random_case(n, K, seed, mixed=True):
    """n points in a 60 m x 60 m x 40 m box at the UTM-like origin, K regions that each hold a part of them"""
    rng = np.random.default_rng(seed)
    pts = ORIGIN + rng.random((n, 3)) * np.array([60.0, 60.0, 40.0])
    labels = rng.choice(np.array([0.0, 2.0, 15.0, 16.0]), n)
    regions = np.zeros((K, 4))
    kinds = (rng.random(K) < 0.5).astype(np.int32) if mixed else np.zeros(K, dtype=np.int32)
    for k in range(K):
        c = ORIGIN[:2] + rng.random(2) * 60.0
        if kinds[k] == DISC:
            regions[k] = [c[0], c[1], rng.uniform(0.5, 25.0), rng.standard_normal()]   # the 4th entry is not read
        else:
            w = rng.uniform(0.5, 30.0, 2)
            regions[k] = [c[0] - w[0], c[1] - w[1], c[0] + w[0], c[1] + w[1]]
    return pts, labels, regions, kinds


# ---- (b) exact boundaries --------------------------------------------------------------------------------------------
TRIPLES = ((3, 4, 5), (-5, 12, 13), (4, -3, 5), (-12, -5, 13), (0, 5, 5), (-13, 0, 13))
SCALES = (0.25, 1.0, 7.5)


def boundary_case():
    """(pts, labels, regions, kinds, claims): claims = (region, point, is_member) the definition states outright.
    Discs: centre + s (a, b) lies exactly on the circle of r = s c for a Pythagorean (a, b, c) -- every product and the
    sum are exact -- so it is a member at r and not at nextafter(r, 0).  Boxes: a point equal to each bound is inside,
    one ulp outside each bound is not."""
    pts, regions, kinds, claims = [], [], [], []
    for s in SCALES:
        for hyp in (5, 13):
            r = hyp * s
            k_in, k_out = len(regions), len(regions) + 1
            regions += [[CENTRE[0], CENTRE[1], r, 0.0], [CENTRE[0], CENTRE[1], np.nextafter(r, 0.0), 0.0]]
            kinds += [DISC, DISC]
            for a, b, c in TRIPLES:
                if c != hyp:
                    continue
                claims += [(k_in, len(pts), True), (k_out, len(pts), False)]
                pts.append([CENTRE[0] + s * a, CENTRE[1] + s * b, 150.0 + len(pts)])
    lo, hi = CENTRE + np.array([-17.25, 3.5]), CENTRE + np.array([8.125, 40.0])
    mid = (lo + hi) / 2
    kb = len(regions)
    regions.append([lo[0], lo[1], hi[0], hi[1]])
    kinds.append(BOX)
    inf = np.inf
    for on, off in (((lo[0], mid[1]), (np.nextafter(lo[0], -inf), mid[1])), ((hi[0], mid[1]), (np.nextafter(hi[0], inf), mid[1])),
                    ((mid[0], lo[1]), (mid[0], np.nextafter(lo[1], -inf))), ((mid[0], hi[1]), (mid[0], np.nextafter(hi[1], inf))),
                    ((lo[0], lo[1]), (np.nextafter(lo[0], -inf), np.nextafter(lo[1], -inf))), ((hi[0], hi[1]), (hi[0], np.nextafter(hi[1], inf)))):
        claims += [(kb, len(pts), True), (kb, len(pts) + 1, False)]
        pts += [[on[0], on[1], -3.0], [off[0], off[1], 1e9]]
    pts = np.array(pts, dtype=np.float64)
    return pts, np.arange(len(pts), dtype=np.float64), np.array(regions), np.array(kinds, dtype=np.int32), claims


def rim_case(chunk):
    """(pts, labels, regions, kinds, claims) for the chunk-level reject: each workgroup's points lie to one side of the
    regions and ONE of them sits exactly on the rim -- the chunk's xy box touches the disc (or box) in that point alone.
    At r it is a member, so the chunk must not be skipped; at nextafter(r, 0) nothing of the chunk is."""
    rng = np.random.default_rng(17)
    cx, cy = CENTRE
    left = np.column_stack([rng.uniform(cx - 40, cx - 5.001, chunk), rng.uniform(cy - 1, cy + 1, chunk), rng.random(chunk)])
    left[chunk // 3] = [cx - 5.0, cy, 1.0]                      # the chunk's largest x: on the circle of r = 5
    above = np.column_stack([rng.uniform(cx - 1, cx + 1, chunk), rng.uniform(cy + 5.001, cy + 40, chunk), rng.random(chunk)])
    above[chunk - 1] = [cx, cy + 5.0, 2.0]                      # the chunk's smallest y
    right = np.column_stack([rng.uniform(cx + 13.001, cx + 50, 17), rng.uniform(cy - 1, cy + 1, 17), rng.random(17)])
    right[0] = [cx + 13.0, cy, 3.0]                             # the (partial) chunk's smallest x: on the circle of r = 13
    pts = np.concatenate([left, above, right])
    i_left, i_above, i_right = chunk // 3, 2 * chunk - 1, 2 * chunk
    regions = np.array([[cx, cy, 5.0, 0.0], [cx, cy, np.nextafter(5.0, 0.0), 0.0], [cx, cy, 13.0, 0.0],
                        [cx, cy, np.nextafter(13.0, 0.0), 0.0], [cx, cy, -5.0, 0.0],
                        [cx - 5.0, cy - 1, cx + 100, cy + 1], [np.nextafter(cx - 5.0, np.inf), cy - 1, cx + 100, cy + 1],
                        [cx - 100, cy - 9, cx + 100, cy + 5.0], [cx - 100, cy - 9, cx + 100, np.nextafter(cy + 5.0, -np.inf)]])
    kinds = np.array([DISC] * 5 + [BOX] * 4, dtype=np.int32)
    claims = [(0, i_left, True), (0, i_above, True), (1, i_left, False), (1, i_above, False), (2, i_right, True),
              (3, i_right, False), (4, i_left, True), (5, i_left, True), (6, i_left, False), (7, i_above, True),
              (8, i_above, False)]
    return pts, np.arange(len(pts), dtype=np.float64), regions, kinds, claims


# ---- (c) contraction -------------------------------------------------------------------------------------------------
def _fl(q):
    return float(q)      # int / int true division: correctly rounded


@functools.lru_cache(maxsize=None)
def contraction_case(draws=1500):
    """(pts, labels, regions, kinds, count): one point and one disc per qualifying draw of default_rng(3) -- x, y within
    20 m of CENTRE where fl(fl(dx^2) + fl(dy^2)) and a singly-rounded dx^2 + fl(dy^2) (or with x and y swapped: what a
    contracted kernel computes) differ, and some r among sqrt(T) and its neighbours has r * r == T, T the smaller sum.  At
    that r the two sums fall on different sides of the comparison: a contracted kernel gets exactly these wrong."""
    rng = np.random.default_rng(3)
    xy = CENTRE + rng.uniform(-20.0, 20.0, (draws, 2))
    keep, radii = [], []
    for i in range(draws):
        dx, dy = float(xy[i, 0] - CENTRE[0]), float(xy[i, 1] - CENTRE[1])
        a, b = dx * dx, dy * dy
        plain = a + b
        fused = [_fl(Fraction(dx) ** 2 + Fraction(b)), _fl(Fraction(dy) ** 2 + Fraction(a))]
        other = [f for f in fused if f != plain]
        if not other:
            continue
        T = min(plain, min(other))
        root = float(np.sqrt(T))
        for r in (root, float(np.nextafter(root, 0.0)), float(np.nextafter(root, np.inf))):
            if r * r == T:
                keep.append(i)
                radii.append(r)
                break
    pts = np.column_stack([xy[keep], 150.0 + np.arange(len(keep))])
    regions = np.column_stack([np.tile(CENTRE, (len(keep), 1)), radii, np.zeros(len(keep))])
    return pts, np.arange(len(keep), dtype=np.float64), regions, np.zeros(len(keep), dtype=np.int32), len(keep)


# ---- (d) non-finite and odd values -----------------------------------------------------------------------------------
def _payload_nan(payload, negative=False, quiet=True):
    u = np.uint64(0x7ff0000000000000 | (0x0008000000000000 if quiet else 0) | payload | (1 << 63 if negative else 0))
    return np.array([u], dtype=np.uint64).view(np.float64)[0]


def nonfinite_case():
    """(pts, labels, regions, kinds): NaN, +-inf, -0.0, a denormal and NaNs with payloads in each of x, y, z and the label,
    among ordinary points; regions with r NaN / +inf / 0 / negative, a NaN centre, boxes with min > max, infinite bounds,
    min == max, and kinds that are neither disc nor box."""
    odd = [np.nan, np.inf, -np.inf, -0.0, 5e-324, _payload_nan(0x1234), _payload_nan(0xbeef, negative=True),
           _payload_nan(0x77, quiet=False)]
    base = np.array([CENTRE[0] + 1.0, CENTRE[1] - 2.0, 151.0])
    pts, labels = [], []
    rng = np.random.default_rng(11)
    for col in range(4):
        for v in odd:
            p, l = base + rng.uniform(-3, 3, 3), 15.0
            if col < 3:
                p[col] = v
            else:
                l = v
            pts.append(p)
            labels.append(l)
            pts.append(base + rng.uniform(-3, 3, 3))      # an ordinary neighbour
            labels.append(float(len(pts)))
    pts.append(np.array([-0.0, -0.0, -0.0]))
    labels.append(-0.0)
    pts.append(np.array([CENTRE[0], CENTRE[1], 0.0]))       # sits on the degenerate regions
    labels.append(7.0)
    cx, cy = CENTRE
    inf, nan = np.inf, np.nan
    rows = [([cx, cy, nan, 0.0], DISC), ([cx, cy, inf, 0.0], DISC), ([cx, cy, 0.0, 0.0], DISC), ([cx, cy, -4.0, 0.0], DISC),
            ([cx, cy, 4.0, nan], DISC), ([nan, cy, 10.0, 0.0], DISC), ([cx, inf, 10.0, 0.0], DISC), ([0.0, 0.0, 0.0, 0.0], DISC),
            ([cx + 5, cy - 5, cx - 5, cy + 5], BOX), ([-inf, -inf, inf, inf], BOX), ([-inf, -inf, -inf, -inf], BOX),
            ([cx, cy, cx, cy], BOX), ([cx - 5, -inf, cx + 5, inf], BOX), ([nan, cy - 5, cx + 5, cy + 5], BOX),
            ([-0.0, -0.0, 0.0, 0.0], BOX), ([cx, cy, inf, 0.0], 2), ([-inf, -inf, inf, inf], -1), ([cx, cy, inf, 0.0], 1 << 30)]
    regions = np.array([r for r, _ in rows], dtype=np.float64)
    kinds = np.array([k for _, k in rows], dtype=np.int32)
    return np.array(pts, dtype=np.float64), np.array(labels, dtype=np.float64), regions, kinds


# ---- the golden fixture ----------------------------------------------------------------------------------------------
def golden_crops(npz):
    """[(name, row [4], kind)] for every crop stored in tests/golden/scan_crops.npz, with its membership bits under
    npz[name + '_bits'] (np.packbits over the tile's rows)"""
    out = []
    for j, r in enumerate(npz["at_radii_used"]):
        for i, c in enumerate(npz["at_centres"]):
            out.append((f"at_{j}_{i}", np.array([c[0], c[1], r, 0.0]), DISC))
    for j, r in enumerate(npz["tower_radii_used"]):
        c = npz["tower_baricentre"]
        out.append((f"tower_{j}", np.array([c[0], c[1], r, 0.0]), DISC))
    lo, hi = npz["two_min"], npz["two_max"]
    out.append(("two", np.array([lo[0], lo[1], hi[0], hi[1]]), BOX))
    return out
