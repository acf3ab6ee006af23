"""Neighbourhood shapes (K22), the part that needs no GPU: the accuracy of the restated Jacobi solver against mpmath at 60
digits (next to np.linalg.eigh on the same matrices), known shapes through the oracle, and the argument checks of the C
entries."""
import ctypes

import mpmath
import numpy as np
import pytest
import torch

import scene_net_amd as sna
from scene_net_amd import _hip

import shape_cases as sc


def _full(c):
    return [[c[0], c[1], c[2]], [c[1], c[3], c[4]], [c[2], c[4], c[5]]]


def _worst_units(C, exact, lam, vec):
    """(worst eigenvalue error, worst residual ||C v - l v|| over the three unit vectors) in units of 2^-53 * ||C||_F"""
    worst_e = worst_r = mpmath.mpf(0)
    for i, c in enumerate(C):
        M = mpmath.matrix(_full([float(x) for x in c]))
        fro = mpmath.sqrt(sum(M[a, b] ** 2 for a in range(3) for b in range(3)))
        if fro == 0:
            continue
        unit = fro * mpmath.mpf(2) ** -53
        for j in range(3):
            l = mpmath.mpf(float(lam[i, j]))
            v = mpmath.matrix([float(x) for x in vec[i, :, j]])
            v = v / mpmath.sqrt(sum(x * x for x in v))
            res = M * v - l * v
            worst_e = max(worst_e, abs(l - exact[i][j]) / unit)
            worst_r = max(worst_r, mpmath.sqrt(sum(x * x for x in res)) / unit)
    return float(worst_e), float(worst_r)


def test_solver_accuracy_against_mpmath():
    """every 8th covariance matrix of ALL case sets (accuracy_matrices: 11 436 of them; the figures in shape_cases.py are
    those of the whole list, measured once; the stride keeps this test at seconds)"""
    C = sc.accuracy_matrices()
    assert len(C) > 10000
    C = C[::8]
    mpmath.mp.dps = 60
    exact = []
    for c in C:
        E, _ = mpmath.eigsy(mpmath.matrix(_full([float(x) for x in c])))
        exact.append(sorted(E[i] for i in range(3)))
    w, v = np.linalg.eigh(np.array([_full(c) for c in C]))
    eigh = _worst_units(C, exact, w, v)
    lam, vec = sc.jacobi(list(C.T), sc.SWEEPS)
    jac = _worst_units(C, exact, lam, vec)
    less = _worst_units(C, exact, *sc.jacobi(list(C.T), sc.SWEEPS - 1))
    print(f"units of 2^-53 ||C||_F: eigh {eigh}, Jacobi at {sc.SWEEPS} sweeps {jac}, at {sc.SWEEPS - 1} sweeps {less}")
    bar = tuple(max(4.0 * e, 8.0) for e in eigh)
    assert jac[0] <= bar[0] and jac[1] <= bar[1], (jac, bar)
    assert less[0] > bar[0] or less[1] > bar[1], "one sweep fewer does not meet the bar: SWEEPS is the smallest that does"
    assert np.all(np.diff(lam, axis=1) >= 0), "ascending"
    assert _hip.SN_SHAPE_SWEEPS == sc.SWEEPS and _hip.SN_SHAPE_NFEAT == sc.NFEAT


def test_jacobi_edge_cases():
    # a diagonal matrix: every rotation skipped, sorted with the vectors carried along; equal values keep index order
    lam, vec = sc.jacobi([np.array([5.0, 2.0]), np.zeros(2), np.zeros(2), np.array([1.0, 2.0]), np.zeros(2),
                          np.array([3.0, 2.0])])
    assert lam.tolist() == [[1.0, 3.0, 5.0], [2.0, 2.0, 2.0]]
    assert vec[0].tolist() == [[0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]] and vec[1].tolist() == np.eye(3).tolist()
    # a huge theta: theta * theta = +inf gives t = 0 -- the element is dropped, nothing else moves
    lam, vec = sc.jacobi([np.array([1.0]), np.array([1e-200]), np.zeros(1), np.array([1e160]), np.zeros(1), np.array([2.0])])
    assert lam.tolist() == [[1.0, 2.0, 1e160]] and np.isfinite(vec).all()
    # the sign rule
    v = sc.unit_and_sign(np.array([[0.0, 0.0, -2.0], [0.0, -3.0, 0.0], [-4.0, 0.0, 0.0], [1.0, -1.0, 0.0], [3.0, 0.0, 4.0]]))
    assert v[:4].tolist() == [[0.0, 0.0, 1.0], [0.0, 1.0, 0.0], [1.0, 0.0, 0.0], [-1.0 / np.sqrt(2.0), 1.0 / np.sqrt(2.0), 0.0]]
    assert v[4].tolist() == [3.0 / 5.0, 0.0, 4.0 / 5.0]


def test_normal_of_an_exact_plane_within_the_quantisation_bound():
    """Offsets are rounded to the quantum radius / 65536, so a member moves by at most d = 2^-17 * radius per axis, sqrt(3) d
    in length; the coordinates themselves sit within 1e-9 of the plane (an ulp of a UTM northing).  With centred exact
    positions x_i (in the plane) and centred displacements e_i, |e_i| <= eta = 2 (sqrt(3) d + 1e-9), the computed normal v =
    cos(a) n + sin(a) w (w a unit vector in the plane) has v' C' v <= n' C' n <= eta^2, and by Minkowski's inequality
    sin(a) sqrt(mean (x_i . w)^2) <= sqrt(v' C' v) + sqrt(mean (e_i . v)^2) <= 2 eta.  So sin(a) <= 2 eta / sqrt(l1), l1 the
    smaller in-plane eigenvalue of the exact members' covariance.  1e-9 is added for the rounding of covariance and solver
    (2^-18.6 units squared against eigenvalues of 1e8 units squared)."""
    radius = 1.0
    P, n = sc.tilted_plane((0.3, -0.2, 0.9))
    count, mom, eig, normal, axis, feat = sc.shape_oracle(P, radius)
    Q = P - sc.ORIGIN
    member = sc.squared_distances(P) <= radius * radius
    ok = count >= 10
    assert ok.sum() > 1400 and np.array_equal(member.sum(axis=1), count)
    a = np.cross(n, [1.0, 0.0, 0.0])
    a /= np.linalg.norm(a)
    uv = np.stack([Q @ a, Q @ np.cross(n, a)], axis=1)
    w = member / member.sum(axis=1, keepdims=True)
    mean = w @ uv
    cuu, cvv, cuv = (w @ (uv[:, i] * uv[:, j]) - mean[:, i] * mean[:, j] for i, j in ((0, 0), (1, 1), (0, 1)))
    l1 = 0.999 * ((cuu + cvv) / 2.0 - np.sqrt(((cuu - cvv) / 2.0) ** 2 + cuv ** 2))
    eta = 2.0 * (np.sqrt(3.0) * 2.0 ** -17 * radius + 1e-9)
    bound = 2.0 * eta / np.sqrt(l1[ok]) + 1e-9
    sin_a = np.linalg.norm(np.cross(normal[ok], n), axis=1)
    print(f"worst sin(angle) {sin_a.max():.3e}, worst ratio to its bound {np.max(sin_a / bound):.3f}, bounds up to {bound.max():.3e}")
    assert np.all(sin_a <= bound) and bound.max() < 1e-3
    assert np.all(normal[ok, 2] > 0) and np.all(feat[ok, 2] < 1e-8), "nothing out of the plane"
    assert np.all(np.abs(feat[ok, 4] - (1.0 - n[2])) < 1e-3), "verticality is 1 - |n_z|"


def test_line_plane_and_ball_have_their_feature_dominant():
    for k, (name, (P, radius)) in enumerate(sc.known_shapes().items()):
        count, mom, eig, normal, axis, feat = sc.shape_oracle(P, radius)
        ok = count >= 0.8 * count.max()              # whole neighbourhoods: at its rim a plane patch is a half disc
        assert ok.sum() > 100 and count.max() >= 30, name
        top = np.argmax(feat[ok, :3], axis=1)
        print(f"{name}: {ok.sum()} rows, {sc.FEATURE_NAMES[k]} dominant in {(top == k).mean():.3f}, median {np.median(feat[ok, k]):.3f}")
        assert (top == k).mean() > 0.95, name
        assert np.all(np.abs(feat[ok, 0] + feat[ok, 1] + feat[ok, 2] - 1.0) < 1e-12), "the three shares sum to 1"
        assert np.all((feat[ok] >= 0.0) & (feat[ok] <= 1.0))
        if name == "line":
            d = np.array([1.0, 1.0, 4.0]) / np.sqrt(18.0)
            assert np.all(np.abs(axis[ok] @ d) > 0.999) and np.all(feat[ok, 5] > 0.9), "upright: |axis_z| is 4 / sqrt(18)"


def test_oracle_properties():
    P, r = sc.blobs_case(2)[0], sc.BLOB_RADIUS[2]
    count, mom, eig, normal, axis, feat = sc.oracle_of_blobs(2)
    assert (count >= 3).sum() > 1400 and (count < 3).sum() > 100 and count.min() >= 1
    live = count >= 3
    assert np.isnan(eig[~live]).all() and np.isnan(feat[~live]).all() and not np.isnan(feat[live]).any()
    assert np.all(np.abs(np.linalg.norm(normal[live], axis=1) - 1.0) < 1e-15) and np.all(normal[live, 2] >= 0)
    assert np.all(np.abs(np.sum(normal[live] * axis[live], axis=1)) < 1e-12), "normal and axis are orthogonal"
    # against numpy's own covariance and eigh, in coordinate units
    for i in np.flatnonzero(live)[:50]:
        d = P - P[i]
        nb = P[(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2] <= r * r] - P[i]
        w = np.linalg.eigvalsh(np.cov(nb.T, bias=True))
        assert np.allclose(eig[i], w, rtol=1e-3, atol=1e-3 * w[2]), "the quantum is 2^-16 of the radius"
    # a permutation of the rows permutes count and moments and nothing else
    perm = np.random.default_rng(1).permutation(len(P))
    c2, m2 = sc.moments_oracle(np.ascontiguousarray(P[perm]), r)
    assert np.array_equal(c2, count[perm]) and np.array_equal(m2, mom[perm])
    # half-way offsets round to even
    T, tr = sc.tie_case()
    tc, tm = sc.moments_oracle(T, tr)
    k = np.rint((T[1:] - T[0]) * 65536.0)
    assert np.all(k % 2 == 0) and np.array_equal((T[1:] - T[0]) * 65536.0 * 2.0 % 2.0, np.ones_like(k)), "k + 1/2, rounded to even"
    assert tc[0] == 401 and np.array_equal(tm[0, :3], k.sum(axis=0).astype(np.int64))
    # the ring: S2 beyond 32 bits
    R, rr = sc.rim_ring_case()
    rc, rm = sc.moments_oracle(R, rr)
    assert rc[0] == len(R) == 2998 and rm[0, 3] > 2 ** 41 and rm[0, 6] > 2 ** 41 and rm[0, 8] > 2 ** 41


def test_chunk_points_and_ws_bytes():
    lib = _hip.load()
    assert lib.sn_shape_chunk_points() == _hip.shape_chunk_points() == 256
    for total, B, cells in ((0, 1, 1), (-5, 1, 1), ((1 << 30) + 1, 1, 1), (10, 0, 1), (10, -1, 1), (10, 1, 0),
                            (10, 1, (1 << 22) + 1), (10, 3, (1 << 22) // 3 + 1), (10, 1 << 23, 1)):
        assert lib.sn_shape_ws_bytes(total, B, cells) == 0, (total, B, cells)
    a, b = lib.sn_shape_ws_bytes(1000, 1, 10), lib.sn_shape_ws_bytes(2000, 1, 10)
    assert 0 < a < b and b - a <= 1000 * 36 + 64
    assert lib.sn_shape_ws_bytes(1000, 1, 100) - a == 90 * 8 and lib.sn_shape_ws_bytes(1 << 30, 1, 1 << 22) > 0
    with pytest.raises(_hip.HipLibraryError):
        _hip.shape_ws_bytes(0, 1, 1)


def test_argument_checks_need_no_gpu():
    lib = _hip.load()
    buf = ctypes.create_string_buffer(512)
    base = (ctypes.addressof(buf) + 15) // 16 * 16
    p = ctypes.c_void_p(base)
    off = lambda d: ctypes.c_void_p(base + d)   # noqa: E731
    big = ctypes.c_size_t(1 << 40)

    def shape(pts=p, offsets=p, total=100, B=2, radius=2.0, min_points=3, flags=0, lo=p, dx=4, dy=4, dz=4, mult=1, ws=p,
              ws_bytes=big, count=p, moments=p, eig=p, normal=p, axis=p, feat=p):
        return lib.sn_shape_points(pts, offsets, total, B, radius, min_points, flags, lo, dx, dy, dz, mult, ws, ws_bytes, count,
                                   moments, eig, normal, axis, feat, None)

    for name in ("pts", "offsets", "lo", "ws", "count"):
        assert shape(**{name: None}) == -1, name
        assert b"null" in lib.sn_last_error()
    for kw, word in (({"total": 0}, b"total"), ({"total": -3}, b"total"), ({"B": 0}, b"B must"), ({"B": -1}, b"B must"),
                     ({"min_points": 2}, b"min_points"), ({"min_points": 0}, b"min_points"), ({"min_points": -4}, b"min_points"),
                     ({"radius": 0.0}, b"radius"), ({"radius": -1.0}, b"radius"), ({"radius": float("nan")}, b"radius"),
                     ({"radius": float("inf")}, b"radius"), ({"dx": 0}, b"dims"), ({"dy": -1}, b"dims"), ({"dz": 0}, b"dims"),
                     ({"mult": 0}, b"mult"), ({"flags": 1}, b"flags"), ({"flags": -8}, b"flags")):
        assert shape(**kw) == -1, kw
        assert word in lib.sn_last_error(), (kw, lib.sn_last_error())
    for kw, word in (({"total": (1 << 30) + 1}, b"2^30"), ({"dx": 1 << 11, "dy": 1 << 11, "dz": 2}, b"cells"),
                     ({"B": 3, "dx": 128, "dy": 128, "dz": 128}, b"cells"), ({"radius": 1e-160}, b"radius"),
                     ({"radius": 1e160}, b"radius")):
        assert shape(**kw) == -2, kw
        assert word in lib.sn_last_error(), (kw, lib.sn_last_error())
    for name, d in (("pts", 4), ("offsets", 4), ("lo", 4), ("ws", 8), ("count", 2), ("moments", 4), ("eig", 4), ("normal", 4),
                    ("axis", 4), ("feat", 4)):
        assert shape(**{name: off(d)}) == -1, name
        assert b"aligned" in lib.sn_last_error()
    need = lib.sn_shape_ws_bytes(100, 2, 64)
    assert need > 0 and shape(ws_bytes=ctypes.c_size_t(need - 1)) == -1
    assert b"sn_shape_ws_bytes" in lib.sn_last_error()
    args = (p, p, 100, 2, 2.0, 3, 0, p, 4, 4, 4, 1, p, big, p, p, p, p, p, p)
    assert lib.sn_shape_points_launches(*args, 0, 3, None) == -1 and lib.sn_shape_points_launches(*args, 2, 6, None) == -1
    assert lib.sn_shape_points_launches(*args, 3, 2, None) == -1 and b"first" in lib.sn_last_error()


def test_cpu_tensors_and_limits_raise():
    pts = torch.zeros(8, 3, dtype=torch.float64)
    for call in (lambda: sna.shape_features(pts, 1.0), lambda: sna.estimate_normals(pts, 1.0),
                 lambda: sna.select_by_shape(pts, 1.0, "linearity", minimum=0.5)):
        with pytest.raises(sna.HipLibraryError, match="no CPU path"):
            call()
    with pytest.raises(ValueError, match="exactly one"):
        sna.select_by_shape(pts, 1.0, "linearity")
    with pytest.raises(ValueError, match="no feature"):
        sna.select_by_shape(pts, 1.0, "roundness", minimum=0.5)
    for name in ("PointShapes", "shape_features", "estimate_normals", "select_by_shape", "shape_colors"):
        assert hasattr(sna, name) and name in sna.__all__
    assert sna.PointShapes.FEATURE_NAMES == sc.FEATURE_NAMES
