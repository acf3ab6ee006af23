"""Neighbourhood shapes (K22): the numpy oracle -- brute force over all pairs with the literal formulas of
include/scenenet_hip.h: np.rint, int64 sums, then covariance, cyclic Jacobi, sort, sign rule and features restated operation
for operation (elementwise numpy: + - * / and sqrt are correctly rounded, as the device's) -- and the point sets the host
and GPU tests share (those of dbscan_cases.py / knn_cases.py, m <= 3000).  Everything is compared bit for bit.

Solver accuracy, measured once over ALL 11 436 covariance matrices of accuracy_matrices() against mpmath.eigsy at 60
digits, in units of 2^-53 * ||C||_F, worst over the matrices (test_shape_host.py::test_solver_accuracy_against_mpmath
measures every 8th again and asserts the bar):
                         eigenvalues   residuals ||C v - l v||
    np.linalg.eigh            11.30         12.04
    Jacobi, 2 sweeps        2.2e+13       2.8e+14
    Jacobi, 3 sweeps        5.6e+05       3.4e+10
    Jacobi, 4 sweeps           3.39          3.41
    Jacobi, 5 and 6 sweeps     3.39          3.41     (the same bits as 4)
The bar is 4 x eigh's figure and not below 8 units, i.e. 45.2 and 48.1: 4 sweeps is the smallest count that meets it, and
SN_SHAPE_SWEEPS is 4."""
import functools

import numpy as np

from dbscan_cases import ORIGIN, blobs_case, nonfinite_case, seam_case, small_cloud, squared_distances  # noqa: F401
from knn_cases import BLOB_RADIUS

SWEEPS = 4                      # SN_SHAPE_SWEEPS
NFEAT = 6
FEATURE_NAMES = ("linearity", "planarity", "scattering", "surface_variation", "verticality", "uprightness")
EIGH_UNITS = (11.30, 12.04)     # np.linalg.eigh, worst eigenvalue error and residual (units above) over all matrices
JACOBI_UNITS = (3.39, 3.41)     # this solver at SWEEPS


# ---- the walk: count and moments --------------------------------------------------------------------------------------
def moments_oracle(P, radius):
    """(count [m] i32, moments [m,9] i64) of ONE tile: members q (p included) with (dx*dx + dy*dy) + dz*dz <= radius*radius,
    f = rint(fl(q - p) * inv), inv = 65536.0 / radius"""
    m = P.shape[0]
    inv = 65536.0 / radius
    r2 = radius * radius
    count = np.zeros(m, dtype=np.int32)
    mom = np.zeros((m, 9), dtype=np.int64)
    for r0 in range(0, m, 256):
        rows = slice(r0, min(r0 + 256, m))
        with np.errstate(all="ignore"):
            mask = squared_distances(P, rows) <= r2
            f = [np.where(mask, np.rint((P[None, :, a] - P[rows, a][:, None]) * inv), 0.0).astype(np.int64) for a in range(3)]
        count[rows] = mask.sum(axis=1)
        for a in range(3):
            mom[rows, a] = f[a].sum(axis=1)
        for j, (a, b) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
            mom[rows, 3 + j] = (f[a] * f[b]).sum(axis=1)
    return count, mom


# ---- the solver ---------------------------------------------------------------------------------------------------------
def covariance(count, mom):
    """the six C_ab (xx, xy, xz, yy, yz, zz) in fixed-point units squared, each [m] f64; rows with count 0 give NaN"""
    with np.errstate(all="ignore"):
        n = count.astype(np.float64)
        mean = [mom[:, a].astype(np.float64) / n for a in range(3)]
        pairs = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
        return [mom[:, 3 + j].astype(np.float64) / n - mean[a] * mean[b] for j, (a, b) in enumerate(pairs)]


def _rotate(A, V, p, q, r):
    """one rotation on the pair (p, q), r the third index; A: dict of the six elements by sorted index pair, V[k][j]"""
    key = lambda i, j: (min(i, j), max(i, j))   # noqa: E731
    app, aqq, apq, arp, arq = A[(p, p)], A[(q, q)], A[(p, q)], A[key(r, p)], A[key(r, q)]
    skip = apq == 0.0
    with np.errstate(all="ignore"):
        theta = (aqq - app) / (2.0 * apq)
        mag = np.where(theta < 0.0, -theta, theta)
        root = np.sqrt(theta * theta + 1.0)
        u = 1.0 / (mag + root)
        t = np.where(theta < 0.0, -u, u)
        c = 1.0 / np.sqrt(t * t + 1.0)
        s = t * c
        h = t * apq
        new = {(p, p): app - h, (q, q): aqq + h, (p, q): np.zeros_like(apq), key(r, p): c * arp - s * arq,
               key(r, q): s * arp + c * arq}
        for k, v in new.items():
            A[k] = np.where(skip, A[k], v)
        for k in range(3):
            a, b = V[k][p], V[k][q]
            V[k][p] = np.where(skip, a, c * a - s * b)
            V[k][q] = np.where(skip, b, s * a + c * b)


def jacobi(C, sweeps=SWEEPS):
    """(lam [m,3] ascending, vec [m,3,3] with vec[:, :, j] the vector of lam[:, j]) -- not yet normalised or signed.
    C: the six elements (xx, xy, xz, yy, yz, zz), each [m]"""
    C = [np.asarray(c, dtype=np.float64) for c in C]
    m = C[0].shape[0]
    A = {(0, 0): C[0].copy(), (0, 1): C[1].copy(), (0, 2): C[2].copy(), (1, 1): C[3].copy(), (1, 2): C[4].copy(),
         (2, 2): C[5].copy()}
    V = [[np.full(m, 1.0 if k == j else 0.0) for j in range(3)] for k in range(3)]
    for _ in range(sweeps):
        _rotate(A, V, 0, 1, 2)
        _rotate(A, V, 0, 2, 1)
        _rotate(A, V, 1, 2, 0)
    lam = [A[(0, 0)], A[(1, 1)], A[(2, 2)]]
    for i, j in ((0, 1), (1, 2), (0, 1)):       # swap only where the left value is greater
        sw = lam[i] > lam[j]
        lam[i], lam[j] = np.where(sw, lam[j], lam[i]), np.where(sw, lam[i], lam[j])
        for k in range(3):
            V[k][i], V[k][j] = np.where(sw, V[k][j], V[k][i]), np.where(sw, V[k][i], V[k][j])
    vec = np.stack([np.stack(V[k], axis=1) for k in range(3)], axis=1)
    return np.stack(lam, axis=1), vec


def unit_and_sign(v):
    """v [m,3] / sqrt((x*x + y*y) + z*z), negated where z < 0, or z == 0 and y < 0, or z == y == 0 and x < 0"""
    with np.errstate(all="ignore"):
        x, y, z = v[:, 0], v[:, 1], v[:, 2]
        length = np.sqrt((x * x + y * y) + z * z)
        x, y, z = x / length, y / length, z / length
        flip = (z < 0.0) | ((z == 0.0) & ((y < 0.0) | ((y == 0.0) & (x < 0.0))))
        return np.stack([np.where(flip, -x, x), np.where(flip, -y, y), np.where(flip, -z, z)], axis=1)


def solve(count, mom, radius, min_points=3, sweeps=SWEEPS):
    """(eig [m,3], normal [m,3], axis [m,3], feat [m,6]) from count and moments, NaN rows as the header says"""
    unit = radius / 65536.0
    unit2 = unit * unit
    lam, vec = jacobi(covariance(count, mom), sweeps)
    with np.errstate(all="ignore"):
        dead = (count < min_points) | ~(lam[:, 2] > 0.0)
        eig = lam * unit2
        normal, axis = unit_and_sign(vec[:, :, 0]), unit_and_sign(vec[:, :, 2])
        c0, c1, c2 = (np.where(eig[:, j] < 0.0, 0.0, eig[:, j]) for j in range(3))
        nz, az = normal[:, 2], axis[:, 2]
        feat = np.stack([(c2 - c1) / c2, (c1 - c0) / c2, c0 / c2, c0 / ((c0 + c1) + c2), 1.0 - np.where(nz < 0.0, -nz, nz),
                         np.where(az < 0.0, -az, az)], axis=1)
    for out in (eig, normal, axis, feat):
        out[dead] = np.nan
    return eig, normal, axis, feat


def shape_oracle(P, radius, min_points=3):
    """(count, moments, eig, normal, axis, feat) of ONE tile"""
    count, mom = moments_oracle(P, radius)
    return (count, mom) + solve(count, mom, radius, min_points)


def batch_oracle(tiles, radius, min_points=3, pad=0):
    """the oracle of every tile, packed; `pad` rows beyond offsets[B]: count 0, zero moments, NaN"""
    outs = [shape_oracle(np.asarray(P, dtype=np.float64).reshape(-1, 3), radius, min_points) for P in tiles if len(P)]
    if pad:
        outs.append((np.zeros(pad, np.int32), np.zeros((pad, 9), np.int64)) +
                    tuple(np.full((pad, c), np.nan) for c in (3, 3, 3, NFEAT)))
    return tuple(np.concatenate([o[j] for o in outs]) for j in range(6))


@functools.lru_cache(maxsize=None)
def oracle_of_blobs(which):
    return shape_oracle(blobs_case(which)[0], BLOB_RADIUS[which])


# ---- point sets ---------------------------------------------------------------------------------------------------------
def tie_case():
    """(P, radius = 1): a centre and neighbours at offsets that are exact ODD multiples of 2^-17, i.e. f = k + 1/2 exactly:
    rint must round them to the even neighbour.  Small integer-ish coordinates keep every difference exact."""
    rng = np.random.default_rng(17)
    k = rng.integers(-30000, 30000, (400, 3))
    off = (2 * k + 1) * 2.0 ** -17                   # |off| < 0.46: (2k+1) / 2 after the scaling by 65536
    P = np.concatenate([np.zeros((1, 3)), off]) + np.array([4.0, 8.0, 2.0])
    return np.ascontiguousarray(P), 1.0


def rim_ring_case(m=3000):
    """(P, radius = 3): a centre and m - 1 points just inside the rim of its radius on three great circles: for the centre
    S2 is about m * 65536^2 / 3 per axis, far beyond 2^32; the ring points see one another too"""
    t = np.linspace(0.0, 2.0 * np.pi, (m - 1) // 3, endpoint=False)
    c, s, z = np.cos(t) * 2.999, np.sin(t) * 2.999, np.zeros_like(t)
    ring = np.concatenate([np.stack([c, s, z], 1), np.stack([z, c, s], 1), np.stack([s, z, c], 1)])
    return np.ascontiguousarray(np.concatenate([np.zeros((1, 3)), ring]) + ORIGIN), 3.0


def line_lattice(m=60):
    """exactly collinear: steps of (0.25, 0.5, 0.125) from ORIGIN, every coordinate a dyadic rational"""
    return np.ascontiguousarray(ORIGIN + np.arange(m)[:, None] * np.array([0.25, 0.5, 0.125]))


def plane_lattice(n=14):
    """exactly planar: the lattice i * (0.5, 0, 0.25) + j * (0, 0.5, 0.125) -- normal along (-0.5, -0.25, 1)"""
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    P = i.reshape(-1, 1) * np.array([0.5, 0.0, 0.25]) + j.reshape(-1, 1) * np.array([0.0, 0.5, 0.125])
    return np.ascontiguousarray(ORIGIN + P)


def few_neighbours_case():
    """(P, radius = 1): isolated groups of 1, 2, 3, 4 and 5 points 50 m apart: counts 1 .. 5 against min_points 3 and 5"""
    rng = np.random.default_rng(31)
    parts = [np.array([50.0 * g, 0.0, 0.0]) + rng.random((g + 1, 3)) * 0.5 for g in range(5)]
    return np.ascontiguousarray(ORIGIN + np.concatenate(parts)), 1.0


def tilted_plane(normal, m=1500, seed=3, spread=4.0):
    """m points on the plane through ORIGIN with unit normal `normal`, to within the rounding of the coordinates"""
    rng = np.random.default_rng(seed)
    n = np.asarray(normal, dtype=np.float64)
    n = n / np.linalg.norm(n)
    a = np.cross(n, [1.0, 0.0, 0.0] if abs(n[0]) < 0.9 else [0.0, 1.0, 0.0])
    a /= np.linalg.norm(a)
    b = np.cross(n, a)
    uv = (rng.random((m, 2)) - 0.5) * spread
    return np.ascontiguousarray(ORIGIN + uv[:, :1] * a + uv[:, 1:] * b), n


def known_shapes():
    """{name: (P, radius)}: a line along (1, 1, 4) with 1 cm of noise, a plane with 1 cm of noise, a ball"""
    rng = np.random.default_rng(9)
    d = np.array([1.0, 1.0, 4.0]) / np.sqrt(18.0)
    line = ORIGIN + np.linspace(-3.0, 3.0, 600)[:, None] * d + rng.standard_normal((600, 3)) * 0.01
    plane = tilted_plane((0.2, -0.1, 1.0), 1500, 4)[0] + rng.standard_normal((1500, 3)) * 0.01
    ball = ORIGIN + rng.standard_normal((1500, 3)) * 0.8
    return {"line": (line, 1.0), "plane": (plane, 1.0), "ball": (ball, 1.0)}


def accuracy_matrices():
    """[n, 6] f64: the covariance matrices (fixed-point units squared) the solver's accuracy is measured on -- every row
    with at least 3 members of the four blob sets, the seam case, the non-finite case, the lattices, the ring, the tie
    case and the known shapes"""
    sets = [(blobs_case(w)[0], BLOB_RADIUS[w]) for w in range(4)]
    sets += [(seam_case(2.0 * (1.0 + 2.0 ** -20))[0], 2.0), (nonfinite_case()[0], 1.2), (line_lattice(), 1.5),
             (plane_lattice(), 1.2), rim_ring_case(900), tie_case()] + list(known_shapes().values())
    out = []
    for P, r in sets:
        count, mom = moments_oracle(P, r)
        C = np.stack(covariance(count, mom), axis=1)
        out.append(C[count >= 3])
    return np.concatenate(out)
