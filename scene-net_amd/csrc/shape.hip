// K22 -- the shape of a point's neighbourhood: the covariance of every member within a radius, its eigenvalues and
// eigenvectors (normal, principal axis) and the eigenfeatures linearity, planarity, scattering, surface variation,
// verticality and uprightness (sn_shape_points).
// replaces: nothing in the reference (unit_vector / angle_between in utils/pcd_processing.py only orient crops): this is
//           the other half of "a point's neighbourhood" next to K21's distances, and this project's own definition.
//
// Definition (normative, include/scenenet_hip.h): the neighbourhood of row p is p and every row q of its tile with
// (dx*dx + dy*dy) + dz*dz <= radius*radius, K21's candidate test in K21's literal form (this file is built with
// -ffp-contract=off), no cap, duplicates included.  Every member contributes f_a = rint(fl(q_a - p_a) * inv), inv = 65536
// / radius from the host, to nine int64 moments S1[3], S2[6]: integer sums, so the order of rows inside a cell, the grid
// and the order of the rows in the array do not show in any bit.  Covariance, cyclic Jacobi with SN_SHAPE_SWEEPS sweeps,
// the sort, the sign rule and the features are fp64 operations rounded once each, + - * / sqrt only, in the header's order.
//
// The rows are counting-sorted into the cell grid of cell_grid.h exactly as knn.hip sorts them -- one text there for the
// bodies of launches 0 to 3, the layout of the sort's arrays and the checks of the grid's arguments -- by launches of this
// file, so that a trace tells the two calls apart:
//   0 zero     the cells' populations (a kernel, not a memset node: DESIGN section 7 K21, "Launches")
//   1 cells    tile and cell of every row, populations (integer atomics); rows that no tile owns get their empty result
//   2 prefix   cell_starts
//   3 scatter  scatter_row
//   4 shape    one thread per row IN CELL ORDER: the 9 runs of the 27 cells as knn_search_kernel walks them, count and
//              the nine moments in registers (32 x 32 -> 64-bit multiply-adds), then the solver in registers, results
//              stored at the row's own index
// The 9-run candidate loop of launch 4 is written out here as in knn_search_kernel: it ran slower through a callback, per
// row and per run.
//
// Bound: launch 4 by the latency of the candidate loads, as K21's launch 4.
#include "common.h"
#include "cell_grid.h"
#include "packed_rows.h"
#include "scan.h"
#include <cmath>

namespace {

constexpr int kThreads = 256;
constexpr int kChunk = kThreads;   // rows per workgroup of launches 1, 3, 4
constexpr int kSweeps = SN_SHAPE_SWEEPS;
constexpr int kFeat = SN_SHAPE_NFEAT;

using sn::live_rows;   // packed_rows.h
using sn::quiet_nan;

struct Outputs {
    int32_t* count;
    int64_t* moments;
    double *eig, *normal, *axis, *feat;
};

// NaN in every solver output of row i
__device__ __forceinline__ void store_nan(const Outputs& o, size_t i) {
    const double n = quiet_nan();
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        if (o.eig) o.eig[i * 3 + a] = n;
        if (o.normal) o.normal[i * 3 + a] = n;
        if (o.axis) o.axis[i * 3 + a] = n;
    }
    if (o.feat) {
#pragma unroll
        for (int a = 0; a < kFeat; ++a) o.feat[i * kFeat + a] = n;
    }
}

// ---- 0: the populations zeroed by a launch of this file
__global__ __launch_bounds__(kThreads) void shape_zero_kernel(int32_t* __restrict__ pop, int cells) {
    zero_population(pop, cells, blockIdx.x * kThreads + threadIdx.x);
}

// ---- 1: the cell key of every row and the cells' populations; the empty result of rows outside every tile
__global__ __launch_bounds__(kThreads) void shape_cells_kernel(const double* __restrict__ pts,
                                                               const int64_t* __restrict__ offsets, int total, int B,
                                                               const double* __restrict__ lo, CellGrid g,
                                                               int32_t* __restrict__ cell_of, int32_t* __restrict__ pop,
                                                               Outputs o) {
    const int m = live_rows(offsets, B, total);
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= total) return;
    if (i >= m) {
        o.count[i] = 0;
        if (o.moments) {
#pragma unroll
            for (int a = 0; a < 9; ++a) o.moments[(size_t)i * 9 + a] = 0;
        }
        store_nan(o, (size_t)i);
        return;
    }
    count_packed_row(pts, offsets, B, lo, g, i, cell_of, pop);
}

// ---- 2: one workgroup: the cells' starts and cursors
__global__ __launch_bounds__(kScanThreads) void shape_prefix_kernel(int32_t* __restrict__ pop, int cells,
                                                                    int32_t* __restrict__ start) {
    __shared__ int64_t s_wave[kScanThreads / 64];
    cell_starts(pop, cells, start, s_wave);
}

// ---- 3: rows into cell order
__global__ __launch_bounds__(kThreads) void shape_scatter_kernel(const double* __restrict__ pts,
                                                                 const int64_t* __restrict__ offsets, int total, int B,
                                                                 const int32_t* __restrict__ cell_of,
                                                                 int32_t* __restrict__ cursor, Row* __restrict__ rows) {
    const int m = live_rows(offsets, B, total);
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i < m) scatter_packed_row(pts, i, m, cell_of, cursor, rows);
}

// ---- 4: the moments and the solver
// One Jacobi rotation on the pair (p, q) of the symmetric matrix whose elements are app, aqq, apq and, with the third
// index r, arp, arq; (vp, vq) are the two columns of the vectors.  The header's formulas, operation for operation.
__device__ __forceinline__ void rotate(double& app, double& aqq, double& apq, double& arp, double& arq, double (&vp)[3],
                                       double (&vq)[3]) {
#pragma clang fp contract(off)
    if (apq == 0.0) return;
    const double theta = (aqq - app) / (2.0 * apq);
    const double mag = theta < 0.0 ? -theta : theta;
    const double root = sqrt(theta * theta + 1.0);          // (+inf for a huge theta: t = 0)
    const double u = 1.0 / (mag + root);
    const double t = theta < 0.0 ? -u : u;
    const double c = 1.0 / sqrt(t * t + 1.0);
    const double s = t * c;
    const double h = t * apq;
    app = app - h;
    aqq = aqq + h;
    apq = 0.0;
    const double rp = arp, rq = arq;
    arp = c * rp - s * rq;
    arq = s * rp + c * rq;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double a = vp[k], b = vq[k];
        vp[k] = c * a - s * b;
        vq[k] = s * a + c * b;
    }
}

// v / sqrt((x*x + y*y) + z*z), then the sign rule: n_z >= 0; n_z == 0: n_y >= 0; both 0: n_x > 0
__device__ __forceinline__ void unit_and_sign(double (&v)[3]) {
#pragma clang fp contract(off)
    const double len = sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
    v[0] = v[0] / len, v[1] = v[1] / len, v[2] = v[2] / len;
    // Bitwise on purpose, and selects, not a branch: with || and && and `if (flip)` the compiler's code restored the
    // unflipped vector on every lane with z >= 0, so z == 0 and y < 0 was never negated
    const bool flip = (v[2] < 0.0) | ((v[2] == 0.0) & ((v[1] < 0.0) | ((v[1] == 0.0) & (v[0] < 0.0))));
    v[0] = flip ? -v[0] : v[0], v[1] = flip ? -v[1] : v[1], v[2] = flip ? -v[2] : v[2];
}

__device__ __forceinline__ void swap_if_greater(double& la, double& lb, double (&va)[3], double (&vb)[3]) {
    if (la > lb) {
        const double t = la;
        la = lb, lb = t;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double w = va[k];
            va[k] = vb[k], vb[k] = w;
        }
    }
}

__global__ __launch_bounds__(kThreads) void shape_moments_kernel(const int64_t* __restrict__ offsets, int total, int B,
                                                                 CellGrid g, double r2, double inv, double unit2,
                                                                 int min_points, const int32_t* __restrict__ start,
                                                                 const Row* __restrict__ rows, Outputs o) {
#pragma clang fp contract(off)
    const int m = live_rows(offsets, B, total);
    const int r = blockIdx.x * kThreads + threadIdx.x;
    if (r >= m) return;
    const Row me = rows[r];
    if ((unsigned)me.cell >= (unsigned)(B * g.cells)) return;   // (never, behind launches 1 to 3 of the same call)
    int count = 0;
    long long sx = 0, sy = 0, sz = 0, sxx = 0, sxy = 0, sxz = 0, syy = 0, syz = 0, szz = 0;
    const int tile = me.cell / g.cells, local = me.cell - tile * g.cells;
    // the 9 runs of knn_search_kernel on the tile's slice of start
    const int32_t* __restrict__ tstart = start + (size_t)tile * g.cells;
    const int cz = local % g.dim[2], t = local / g.dim[2], cy = t % g.dim[1], cx = t / g.dim[1];
    const int zlo = max(cz - 1, 0), zhi = min(cz + 1, g.dim[2] - 1);
    for (int ax = max(cx - 1, 0); ax <= min(cx + 1, g.dim[0] - 1); ++ax)
        for (int ay = max(cy - 1, 0); ay <= min(cy + 1, g.dim[1] - 1); ++ay) {
            const int base = (ax * g.dim[1] + ay) * g.dim[2];
            const int a = max(tstart[base + zlo], 0), b = min(tstart[base + zhi + 1], m);
            for (int j = a; j < b; ++j) {
                const Row q = rows[j];
                const double dx = q.x - me.x, dy = q.y - me.y, dz = q.z - me.z;
                const double xx = dx * dx, yy = dy * dy, zz = dz * dz;
                const double d2 = (xx + yy) + zz;
                if (!(d2 <= r2)) continue;           // (the row itself passes with d2 = 0 unless it is not finite)
                // |dx| <= radius (1 + 2^-51), so |fx| <= 65537: an int32, and a product of two an int64
                const int fx = (int)__builtin_rint(dx * inv), fy = (int)__builtin_rint(dy * inv),
                          fz = (int)__builtin_rint(dz * inv);
                ++count;
                sx += fx, sy += fy, sz += fz;
                sxx += (long long)fx * fx, sxy += (long long)fx * fy, sxz += (long long)fx * fz;
                syy += (long long)fy * fy, syz += (long long)fy * fz, szz += (long long)fz * fz;
            }
        }
    if ((unsigned)me.pos >= (unsigned)total) return;
    const size_t i = (size_t)me.pos;
    o.count[i] = count;
    if (o.moments) {
        int64_t* mo = o.moments + i * 9;
        mo[0] = sx, mo[1] = sy, mo[2] = sz, mo[3] = sxx, mo[4] = sxy, mo[5] = sxz, mo[6] = syy, mo[7] = syz, mo[8] = szz;
    }
    if (!o.eig && !o.normal && !o.axis && !o.feat) return;
    if (count < min_points) {
        store_nan(o, i);
        return;
    }
    // the population covariance in fixed-point units squared
    const double n = (double)count;
    const double mx = (double)sx / n, my = (double)sy / n, mz = (double)sz / n;
    double a00 = (double)sxx / n - mx * mx, a01 = (double)sxy / n - mx * my, a02 = (double)sxz / n - mx * mz;
    double a11 = (double)syy / n - my * my, a12 = (double)syz / n - my * mz, a22 = (double)szz / n - mz * mz;
    double v0[3] = {1.0, 0.0, 0.0}, v1[3] = {0.0, 1.0, 0.0}, v2[3] = {0.0, 0.0, 1.0};
    for (int sweep = 0; sweep < kSweeps; ++sweep) {
        rotate(a00, a11, a01, a02, a12, v0, v1);   // (0, 1), third index 2
        rotate(a00, a22, a02, a01, a12, v0, v2);   // (0, 2), third index 1
        rotate(a11, a22, a12, a01, a02, v1, v2);   // (1, 2), third index 0
    }
    double l0 = a00, l1 = a11, l2 = a22;
    swap_if_greater(l0, l1, v0, v1);
    swap_if_greater(l1, l2, v1, v2);
    swap_if_greater(l0, l1, v0, v1);
    if (!(l2 > 0.0)) {                               // every member coincides with the row
        store_nan(o, i);
        return;
    }
    unit_and_sign(v0);
    unit_and_sign(v2);
    const double e0 = l0 * unit2, e1 = l1 * unit2, e2 = l2 * unit2;
    if (o.eig) o.eig[i * 3] = e0, o.eig[i * 3 + 1] = e1, o.eig[i * 3 + 2] = e2;
    if (o.normal) o.normal[i * 3] = v0[0], o.normal[i * 3 + 1] = v0[1], o.normal[i * 3 + 2] = v0[2];
    if (o.axis) o.axis[i * 3] = v2[0], o.axis[i * 3 + 1] = v2[1], o.axis[i * 3 + 2] = v2[2];
    if (o.feat) {
        const double c0 = e0 < 0.0 ? 0.0 : e0, c1 = e1 < 0.0 ? 0.0 : e1, c2 = e2 < 0.0 ? 0.0 : e2;
        double* f = o.feat + i * kFeat;
        f[0] = (c2 - c1) / c2;
        f[1] = (c1 - c0) / c2;
        f[2] = c0 / c2;
        f[3] = c0 / ((c0 + c1) + c2);
        f[4] = 1.0 - (v0[2] < 0.0 ? -v0[2] : v0[2]);
        f[5] = v2[2] < 0.0 ? -v2[2] : v2[2];
    }
}

// ------------------------------------------------------------------------------------------------------------------ host
// the workspace is the sort's arrays (cell_grid.h) and nothing else
bool layout_of(int64_t total, int64_t B, int64_t cells_per_tile, SortLayout& L) {
    return sort_layout(total, (int64_t)1 << 30, B, cells_per_tile, 0, L);
}

int run(const double* pts, const int64_t* offsets, int64_t total, int B, double radius, int min_points, int flags,
        const double* lo, int dim_x, int dim_y, int dim_z, int64_t mult, void* ws, size_t ws_bytes, int32_t* count,
        int64_t* moments, double* eig, double* normal, double* axis, double* feat, int first, int last, sn_stream_t stream) {
    const char* who = "sn_shape_points";
    if (!pts || !offsets || !lo || !ws || !count)
        return sn::fail(SN_ERR_INVALID_ARG, "%s: null pointer (pts, offsets, lo, ws, count)", who);
    if (total <= 0) return sn::fail(SN_ERR_INVALID_ARG, "%s: total must be positive (got %lld)", who, (long long)total);
    if (B <= 0) return sn::fail(SN_ERR_INVALID_ARG, "%s: B must be positive (got %d)", who, B);
    if (min_points < 3) return sn::fail(SN_ERR_INVALID_ARG, "%s: min_points must be at least 3 (got %d)", who, min_points);
    if (int e = grid_args_valid(who, radius, dim_x, dim_y, dim_z, mult)) return e;
    if (flags != 0) return sn::fail(SN_ERR_INVALID_ARG, "%s: unknown flags %d (none are defined)", who, flags);
    if (total > ((int64_t)1 << 30))
        return sn::fail(SN_ERR_UNSUPPORTED, "%s: total <= 2^30 rows are served (the moments stay inside int64)", who);
    CellGrid g;
    if (int e = grid_of_tiles(who, radius, B, dim_x, dim_y, dim_z, mult, g)) return e;
    if ((uintptr_t)pts % 8 || (uintptr_t)offsets % 8 || (uintptr_t)lo % 8 || (uintptr_t)ws % 16 || (uintptr_t)count % 4 ||
        (uintptr_t)moments % 8 || (uintptr_t)eig % 8 || (uintptr_t)normal % 8 || (uintptr_t)axis % 8 || (uintptr_t)feat % 8)
        return sn::fail(SN_ERR_INVALID_ARG, "%s: pts / offsets / lo / moments / eig / normal / axis / feat must be 8-byte "
                        "aligned, ws 16-byte, count 4-byte", who);
    SortLayout L;
    layout_of(total, B, g.cells, L);
    if (ws_bytes < L.bytes)
        return sn::fail(SN_ERR_INVALID_ARG, "%s: ws holds %zu bytes, %zu needed (sn_shape_ws_bytes)", who, ws_bytes, L.bytes);

    hipStream_t s = sn::as_stream(stream);
    char* w = static_cast<char*>(ws);
    Row* rows = reinterpret_cast<Row*>(w + L.rows);
    int32_t* cell_of = reinterpret_cast<int32_t*>(w + L.cell_of);
    int32_t* start = reinterpret_cast<int32_t*>(w + L.start);
    int32_t* pop = reinterpret_cast<int32_t*>(w + L.pop);
    const int n = (int)total;
    const dim3 grid((unsigned)((n + kThreads - 1) / kThreads)), block(kThreads);
    const double r2 = radius * radius;
    const double inv = 65536.0 / radius;      // one rounding
    const double unit = radius / 65536.0;     // exact: a power of two
    const double unit2 = unit * unit;         // one rounding
    const Outputs o{count, moments, eig, normal, axis, feat};

    if (first <= 1 && last >= 1) {
        hipLaunchKernelGGL(shape_zero_kernel, dim3((unsigned)((L.cells + kThreads - 1) / kThreads)), block, 0, s, pop,
                           (int)L.cells);
        if (int e = sn::check_launch("sn_shape_points(zero)")) return e;
    }
    if (first <= 2 && last >= 2) {
        hipLaunchKernelGGL(shape_cells_kernel, grid, block, 0, s, pts, offsets, n, B, lo, g, cell_of, pop, o);
        if (int e = sn::check_launch("sn_shape_points(cells)")) return e;
    }
    if (first <= 3 && last >= 3) {
        hipLaunchKernelGGL(shape_prefix_kernel, dim3(1), dim3(kScanThreads), 0, s, pop, (int)L.cells, start);
        if (int e = sn::check_launch("sn_shape_points(prefix)")) return e;
    }
    if (first <= 4 && last >= 4) {
        hipLaunchKernelGGL(shape_scatter_kernel, grid, block, 0, s, pts, offsets, n, B, cell_of, pop, rows);
        if (int e = sn::check_launch("sn_shape_points(scatter)")) return e;
    }
    if (first <= 5 && last >= 5) {
        hipLaunchKernelGGL(shape_moments_kernel, grid, block, 0, s, offsets, n, B, g, r2, inv, unit2, min_points, start, rows, o);
        if (int e = sn::check_launch("sn_shape_points(shape)")) return e;
    }
    return SN_OK;
}

}  // namespace

extern "C" int sn_shape_chunk_points(void) { return kChunk; }

extern "C" size_t sn_shape_ws_bytes(int64_t total, int B, int64_t cells_per_tile) {
    SortLayout L;
    return layout_of(total, B, cells_per_tile, L) ? L.bytes : 0;
}

extern "C" int sn_shape_points(const double* pts, const int64_t* offsets, int64_t total, int B, double radius, int min_points,
                               int flags, const double* lo, int dim_x, int dim_y, int dim_z, int64_t mult, void* ws,
                               size_t ws_bytes, int32_t* count, int64_t* moments, double* eig, double* normal, double* axis,
                               double* feat, sn_stream_t stream) {
    return run(pts, offsets, total, B, radius, min_points, flags, lo, dim_x, dim_y, dim_z, mult, ws, ws_bytes, count, moments,
               eig, normal, axis, feat, 1, SN_SHAPE_LAUNCHES, stream);
}

extern "C" int sn_shape_points_launches(const double* pts, const int64_t* offsets, int64_t total, int B, double radius,
                                        int min_points, int flags, const double* lo, int dim_x, int dim_y, int dim_z,
                                        int64_t mult, void* ws, size_t ws_bytes, int32_t* count, int64_t* moments, double* eig,
                                        double* normal, double* axis, double* feat, int first, int last, sn_stream_t stream) {
    if (first < 1 || last > SN_SHAPE_LAUNCHES || first > last)
        return sn::fail(SN_ERR_INVALID_ARG, "sn_shape_points_launches: 1 <= first <= last <= %d", SN_SHAPE_LAUNCHES);
    return run(pts, offsets, total, B, radius, min_points, flags, lo, dim_x, dim_y, dim_z, mult, ws, ws_bytes, count, moments,
               eig, normal, axis, feat, first, last, stream);
}
