"""Point DBSCAN (K10): the numpy oracle -- brute force over all pairs in the literal formula of include/scenenet_hip.h -- and
the point sets its host and GPU tests share.  Everything is compared exactly.  Sets stay at m <= 3000 so that the oracle
runs in seconds."""
import functools
from fractions import Fraction

import numpy as np

ORIGIN = np.array([5.44e5, 4.634e6, 1.5e2])          # UTM-like, as the synthetic tiles
PAIRS = ((10.0, 300), (3.5, 18), (1.6, 5), (2.0, 4))  # eps, min_points
TOWER = 15.0


# ---- the oracle ------------------------------------------------------------------------------------------------------
def squared_distances(P, rows=slice(None)):
    """(dx*dx + dy*dy) + dz*dz for the points `rows` against all: each product and sum rounded once"""
    with np.errstate(all="ignore"):
        d = [P[rows, a][:, None] - P[None, :, a] for a in range(3)]
        return (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]


def neighbours(P, eps):
    """[m, m] bool: the neighbour relation, a point its own neighbour unless a coordinate is NaN or infinite"""
    m = P.shape[0]
    N = np.zeros((m, m), dtype=bool)
    with np.errstate(all="ignore"):
        for r0 in range(0, m, 512):
            N[r0:r0 + 512] = squared_distances(P, slice(r0, r0 + 512)) <= eps * eps
    return N


def rim_pairs(P, eps, rel=1e-9):
    """number of pairs p < q with |d^2 - eps^2| <= rel * eps^2"""
    m, e2, hits = P.shape[0], eps * eps, 0
    for r0 in range(0, m, 512):
        with np.errstate(all="ignore"):
            d2 = squared_distances(P, slice(r0, r0 + 512))
            near = np.abs(d2 - e2) <= rel * e2
        hits += int(np.triu(near, k=r0 + 1).sum())
    return hits


def dbscan_oracle(P, eps, min_points):
    """(cluster [m] int32, n_clusters, stats [K, 3] int64 = n_points, n_core, first core POSITION, core [m] bool)"""
    m = P.shape[0]
    N = neighbours(P, eps)
    core = N.sum(axis=1) >= min_points
    comp = np.full(m, -1, dtype=np.int32)
    K = 0
    for i in range(m):                      # ascending: a cluster is met at its smallest core position
        if core[i] and comp[i] < 0:
            comp[i] = K
            stack = [i]
            while stack:
                p = stack.pop()
                nb = np.flatnonzero(N[p] & core & (comp < 0))
                comp[nb] = K
                stack.extend(nb.tolist())
            K += 1
    cluster = comp.copy()
    for p in np.flatnonzero(~core):
        ids = comp[N[p] & core]
        if ids.size:
            cluster[p] = ids.min()
    stats = np.zeros((K, 3), dtype=np.int64)
    for k in range(K):
        stats[k] = [(cluster == k).sum(), (comp == k).sum(), np.flatnonzero(comp == k)[0]]
    return cluster, K, stats, core


def isin_positions(labels, keep):
    """scan indices of the selected points (np.isin: a NaN label is never selected)"""
    if labels is None:
        return None
    return np.flatnonzero(np.isin(labels, np.asarray(keep, dtype=np.float64))).astype(np.int64)


def finite_bbox(P):
    """(xmin, ymin, zmin, xmax, ymax, zmax) over the finite coordinates, each axis by itself; +inf / -inf for none"""
    out = np.array([np.inf] * 3 + [-np.inf] * 3)
    for a in range(3):
        v = P[:, a][np.isfinite(P[:, a])]
        if v.size:
            out[a], out[3 + a] = v.min(), v.max()
    return out


# ---- (a) blobs with noise at UTM offsets -----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def blobs_case(which, m=1900):
    """(P [m,3], eps, min_points): five Gaussian blobs whose densities straddle min_points, and uniform noise"""
    eps, mp = PAIRS[which]
    rng = np.random.default_rng(100 + which)
    sig = {300: 5.0, 18: 3.0, 5: 1.8, 4: 2.4}[mp]
    nb = m // 6
    parts = []
    for b in range(5):
        c = np.array([b * 7.0 * sig / 2.0 * (1.0 + 0.3 * b), (b % 2) * 3.0 * sig, 0.5 * sig * b])
        parts.append(c + rng.standard_normal((nb, 3)) * sig * (0.6 + 0.25 * b))
    lo = np.min(np.concatenate(parts), axis=0) - 2 * sig
    hi = np.max(np.concatenate(parts), axis=0) + 2 * sig
    parts.append(lo + rng.random((m - 5 * nb, 3)) * (hi - lo))
    P = np.concatenate(parts)
    return np.ascontiguousarray(ORIGIN + P[rng.permutation(m)]), eps, mp


@functools.lru_cache(maxsize=None)
def oracle_of_blobs(which):
    P, eps, mp = blobs_case(which)
    return dbscan_oracle(P, eps, mp)


def golden_towers(tile):
    """the tower points of the golden tile, in scan order"""
    return np.ascontiguousarray(tile[tile[:, 3] == TOWER, :3])


# ---- (b) pairs exactly on the rim ------------------------------------------------------------------------------------
def rim_case(shift=0):
    """(P, eps=5, min_points): integer coordinates at integer UTM offsets, so offsets like (3, 4, 0) and (0, 3, 4) are
    exactly on the rim.  shift = +1 / -1: every second point moved by one ulp up / down in every coordinate, which
    takes each of its rim pairs just out or just in."""
    rng = np.random.default_rng(7)
    P = np.unique(rng.integers(0, 14, (700, 3)), axis=0).astype(np.float64)
    P = P[rng.permutation(len(P))] + ORIGIN
    if shift:
        P[1::2] = np.nextafter(P[1::2], np.inf if shift > 0 else -np.inf)
    return np.ascontiguousarray(P), 5.0, 60


def exact_rim_pairs(P, eps):
    m, hits = P.shape[0], 0
    for r0 in range(0, m, 512):
        hits += int(np.triu(squared_distances(P, slice(r0, r0 + 512)) == eps * eps, k=r0 + 1).sum())
    return hits


# ---- (c) contraction -------------------------------------------------------------------------------------------------
def _fl(q):
    return float(q)      # int / int true division: correctly rounded


def contracted_sums(dx, dy, dz):
    """the values a kernel that contracts a product into a sum may compute for (dx*dx + dy*dy) + dz*dz"""
    xx, yy, zz = dx * dx, dy * dy, dz * dz
    fx, fy, fz = Fraction(dx) ** 2, Fraction(dy) ** 2, Fraction(dz) ** 2
    a, b = _fl(fx + Fraction(yy)), _fl(fy + Fraction(xx))          # fma(dx, dx, yy), fma(dy, dy, xx)
    return [a + zz, b + zz, _fl(fz + Fraction(xx + yy)), _fl(fz + Fraction(a)), _fl(fz + Fraction(b))]


@functools.lru_cache(maxsize=None)
def contraction_case(draws=900):
    """(P, eps=2, min_points=2, pairs, flipped): isolated pairs (100 m apart) whose plain sum and at least one contracted
    sum fall on different sides of eps * eps = 4.  A pair that is a neighbour pair is one cluster of two cores, the others
    are noise: a contracted kernel gets n_clusters wrong.  flipped = the pairs' neighbour verdicts under the plain sum."""
    rng = np.random.default_rng(3)
    pts, verdict = [], []
    for i in range(draws):
        px = 100.0 * len(verdict)
        qx, qy = px + rng.uniform(-1.2, 1.2), rng.uniform(-1.2, 1.2)
        dx, dy = qx - px, qy
        c0 = float(np.sqrt(4.0 - dx * dx - dy * dy))
        for step in range(-6, 7):
            dz = c0
            for _ in range(abs(step)):
                dz = float(np.nextafter(dz, np.inf if step > 0 else -np.inf))
            plain = (dx * dx + dy * dy) + dz * dz
            if any((s <= 4.0) != (plain <= 4.0) for s in contracted_sums(dx, dy, dz)):
                pts += [[px, 0.0, 0.0], [qx, qy, dz]]
                verdict.append(plain <= 4.0)
                break
    return np.array(pts, dtype=np.float64), 2.0, 2, len(verdict), np.array(verdict, dtype=bool)


# ---- (d) cell seams --------------------------------------------------------------------------------------------------
SEAM_LO = ORIGIN.copy()
SEAM_BOUNDS = np.concatenate([SEAM_LO, SEAM_LO + np.array([80.0, 80.0, 80.0])])
SEAM_EPS = 2.0


def _ulps(v, k):
    for _ in range(abs(k)):
        v = float(np.nextafter(v, np.inf if k > 0 else -np.inf))
    return v


def seam_case(side):
    """(P, eps=2, min_points=3) for a grid of cell side `side` from SEAM_LO: per axis, seam j and d in (-1, 0, +1) a point
    a at lo + j * side moved d ulps, with b at a - eps and c at a + eps along that axis: b and c are exactly eps from a
    and sit across the seam.  Alone, a is core (a, b, c) and b, c are its borders; the groups lie on a 7 m lattice, and
    where two of different axes come close the oracle decides as everywhere."""
    pts, g = [], 0
    for axis in range(3):
        for j in (1, 2, 3):
            for d in (-1, 0, 1):
                a = SEAM_LO + np.array([3.0 + 7.0 * (g % 10), 3.0 + 7.0 * (g // 10), 3.0])[np.roll(np.array([2, 0, 1]), axis)]
                a[axis] = _ulps(float(SEAM_LO[axis] + j * side), d)
                b, c = a.copy(), a.copy()
                b[axis] -= SEAM_EPS
                c[axis] += SEAM_EPS
                pts += [a, b, c]
                g += 1
    return np.array(pts, dtype=np.float64), SEAM_EPS, 3


# ---- (e) small constructions -----------------------------------------------------------------------------------------
def chain_case(order, m=3000):
    """m points exactly eps = 2 apart on a line, min_points = 3: one cluster, the two ends are its borders"""
    x = ORIGIN[0] + 2.0 * np.arange(m)
    P = np.column_stack([x, np.full(m, ORIGIN[1]), np.full(m, ORIGIN[2])])
    if order == "descending":
        P = P[::-1]
    elif order == "shuffled":
        P = P[np.random.default_rng(5).permutation(m)]
    return np.ascontiguousarray(P), 2.0, 3


def shared_border_case(order):
    """eps = 1, min_points = 4: A = {0, .25, .5, 1} and B = {3, 3.5, 3.75, 4} are all cores, X = 2 has the neighbours X, 1
    and 3 only: a border that both clusters reach.  Returns (P, eps, min_points, position of X)."""
    A, B, X = [0.0, 0.25, 0.5, 1.0], [3.0, 3.5, 3.75, 4.0], [2.0]
    xs = {"AXB": A + X + B, "BXA": B + X + A, "XBA": X + B + A, "XAB": X + A + B}[order]
    P = np.column_stack([ORIGIN[0] + np.array(xs), np.full(9, ORIGIN[1]), np.full(9, ORIGIN[2])])
    return P, 1.0, 4, xs.index(2.0)


def small_cloud(m, seed, spread=9.0):
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(ORIGIN + rng.random((m, 3)) * spread)


def nonfinite_case():
    """(P, labels, keep, odd): a cloud of 400 ordinary points among which 12 points carry NaN, +inf, -inf or 1e300 in one
    coordinate (positions `odd`); labels hold three kept values, other values and NaNs."""
    rng = np.random.default_rng(23)
    P = small_cloud(412, 29, spread=7.0)
    odd = np.sort(rng.choice(412, 12, replace=False))
    for k, i in enumerate(odd):
        P[i, k % 3] = [np.nan, np.inf, -np.inf, 1e300][k // 3]
    labels = rng.choice(np.array([15.0, 16.0, 2.0, 7.0, np.nan]), 412, p=[0.4, 0.2, 0.2, 0.1, 0.1])
    labels[odd] = 15.0
    return P, labels, (15.0, 16.0, 2.0), odd
