// The cell grid of the neighbourhood kernels, shared by dbscan.hip (K10), knn.hip (K21) and shape.hip (K22): cubic cells of
// side k * eps * (1 + 2^-20), points binned by axis_cell (monotone, clamped), so that two points within eps of each other
// never sit two cells apart and the 27 cells around a point's own hold every neighbour.  One rule, one proof, one text.
//
// The grid is an accelerator only.  Points are counting-sorted into cell order as rows (x, y, z, position, cell): the
// populations per cell (integer atomics, the files' own launch 1), their exclusive prefix and the cursors (cell_starts, one
// workgroup), the rows stored where the cursors say (scatter_row).  With z the fastest cell axis the three cells of one
// (x, y) column are ONE contiguous run of rows: 9 runs per home point (for_candidates).  The order of rows inside a cell depends
// on scheduling (an integer cursor); every result is a count, a minimum, a set union or a function of the candidate SET
// over the runs, so none does.  K21 and K22 sort a packed batch tile by tile (the key is tile * cells + local cell): the
// bodies of their zero, cells and scatter launches, the layout of the sort's arrays and the checks of the grid's arguments
// are at the end of this file; K10 sorts selected positions without tiles, by kernels of its own.  Device text and host
// helpers, no kernels: a trace keeps telling one call's launches from another's.
#pragma once
#include "common.h"
#include "packed_rows.h"
#include "scan.h"
#include <hip/hip_runtime.h>
#include <cmath>

namespace {

constexpr int kScanThreads = 1024;                 // the one-workgroup prefix kernels (their own tile, not scan.h's)
constexpr int kScanItems = 4;
constexpr int64_t kMaxCells = (int64_t)1 << 22;
constexpr double kSideMargin = 1.0 + 0x1p-20;
constexpr double kEpsMin = 1e-150, kEpsMax = 1e150;   // eps * eps is a normal number

struct __attribute__((aligned(16))) Row {
    double x, y, z;
    int pos, cell;
};

struct CellGrid {
    double lo[3];
    double inv;      // 1 / side
    int dim[3];
    int cells;
};

// Cell of coordinate x along one axis: clamp(floor(fl(fl(x - lo) * inv)), 0, dim - 1), NaN -> 0.  Every step is monotone
// non-decreasing in x (IEEE rounding is monotone; inv > 0), so c(x) is.
// Claim: neighbours never sit two cells apart.  A neighbour pair has fl(dx*dx) <= fl(eps*eps) (the sum of non-negative
// terms is no smaller than each, crops.hip's cannot_reach (1)), eps*eps is normal (kEpsMin), so |fl(x1 - x2)| <= eps (1 +
// 2^-51) and |x1 - x2| <= e' = eps (1 + 2^-50).  By monotonicity it suffices that c(x + e') <= c(x) + 1 for real x.
// If c(x) >= dim - 2 the clamp gives it.  If the computed u(x) < 0 then x - lo <= 0 (rounding keeps signs), the exact
// (x + e' - lo) / side < 1 and u(x + e') <= 1 + 2^-51: cell 1 at most.  Otherwise 0 <= u(x) < dim - 2 <= 2^22: the two
// roundings and inv's own (1 / side, one rounding) put u within 2^-50 * 2^22 = 2^-28 of the exact (x - lo) / side, the
// same holds at x + e' (exact value < dim), and the exact values differ by e' / side <= (1 + 2^-50) / ((1 + 2^-20)(1 -
// 2^-52)) < 1 - 2^-21 as side = fl(fl(k eps) (1 + 2^-20)) with k >= 1.  So u(x + e') < u(x) + 1 - 2^-21 + 2^-27 < u(x) + 1
// and the floors differ by one at most.  A clamped point (outside the bounds, infinite) moves towards the others only.
// A NaN coordinate makes the point nobody's neighbour: its cell does not matter.
__device__ __forceinline__ int axis_cell(double x, double lo, double inv, int dim) {
    const double u = (x - lo) * inv;
    if (!(u >= 1.0)) return 0;   // NaN, below the bounds, the first cell
    return u >= (double)(dim - 1) ? dim - 1 : (int)u;
}

__device__ __forceinline__ int cell_of_point(const CellGrid& g, double x, double y, double z) {
    const int cx = axis_cell(x, g.lo[0], g.inv, g.dim[0]);
    const int cy = axis_cell(y, g.lo[1], g.inv, g.dim[1]);
    const int cz = axis_cell(z, g.lo[2], g.inv, g.dim[2]);
    return (cx * g.dim[1] + cy) * g.dim[2] + cz;
}

// the side of a cell, fl(fl(k * eps) * (1 + 2^-20)) in exactly this order (host)
inline double cell_side(double k, double eps) { return k * eps * kSideMargin; }

// One workgroup of kScanThreads.  start[c] = rows in the cells before c, start[cells] = m; pop[c] becomes cell c's cursor.
// s_wave: kScanThreads / 64 slots of LDS
__device__ __forceinline__ void cell_starts(int32_t* pop, int cells, int32_t* start, int64_t* s_wave) {
    int64_t carry = 0;
    for (int t0 = 0; t0 < cells; t0 += kScanThreads * kScanItems) {
        const int c0 = t0 + threadIdx.x * kScanItems;
        int64_t v[kScanItems];
#pragma unroll
        for (int q = 0; q < kScanItems; ++q) v[q] = c0 + q < cells ? pop[c0 + q] : 0;
        const int64_t total = sn::block_exclusive<kScanThreads, kScanItems>(v, s_wave);
#pragma unroll
        for (int q = 0; q < kScanItems; ++q)
            if (c0 + q < cells) {
                start[c0 + q] = (int32_t)(carry + v[q]);
                pop[c0 + q] = (int32_t)(carry + v[q]);
            }
        carry += total;
    }
    if (threadIdx.x == 0) start[cells] = (int32_t)carry;
}

// row r of the m live ones into cell order.  The slot inside a cell is whatever the cursor hands out.
__device__ __forceinline__ void scatter_row(const Row& r, int m, int32_t* __restrict__ cursor, Row* __restrict__ rows) {
    const int slot = atomicAdd(cursor + r.cell, 1);
    if ((unsigned)slot < (unsigned)m) rows[slot] = r;   // (always, behind launches 1 and 2 of the same call)
}

// f(row) for every row of the 27 cells around `cell`, until it returns false: 9 contiguous runs.  knn_search_kernel walks
// the same runs in a loop of its own (measured slower on a callback, per row or per run: DESIGN section 7 K21).
template <typename F>
__device__ __forceinline__ void for_candidates(const CellGrid& g, const int32_t* __restrict__ start,
                                               const Row* __restrict__ rows, int m, int cell, F&& f) {
    const int cz = cell % g.dim[2], t = cell / g.dim[2], cy = t % g.dim[1], cx = t / g.dim[1];
    const int zlo = max(cz - 1, 0), zhi = min(cz + 1, g.dim[2] - 1);
    for (int ax = max(cx - 1, 0); ax <= min(cx + 1, g.dim[0] - 1); ++ax)
        for (int ay = max(cy - 1, 0); ay <= min(cy + 1, g.dim[1] - 1); ++ay) {
            const int base = (ax * g.dim[1] + ay) * g.dim[2];
            const int a = max(start[base + zlo], 0), b = min(start[base + zhi + 1], m);
            for (int j = a; j < b; ++j)
                if (!f(rows[j])) return;
        }
}

// ---- the per-tile counting sort of a packed batch (K21, K22).  The __global__ kernels stay in knn.hip and shape.hip under
// their own names, as wrappers of these bodies; each file keeps the stores of a row that no tile owns.
// launch "zero": population c of `cells` (a kernel, not a memset node: DESIGN section 7 K21, "Launches")
__device__ __forceinline__ void zero_population(int32_t* __restrict__ pop, int cells, int c) {
    if (c < cells) pop[c] = 0;
}

// launch "cells", live row i: its key tile * g.cells + the cell of its point from the tile's own lo, stored and counted
__device__ __forceinline__ void count_packed_row(const double* __restrict__ pts, const int64_t* __restrict__ offsets, int B,
                                                 const double* __restrict__ lo, const CellGrid& g, int i,
                                                 int32_t* __restrict__ cell_of, int32_t* __restrict__ pop) {
    const int b = sn::tile_of_row(offsets, B, i);
    CellGrid t = g;
#pragma unroll
    for (int a = 0; a < 3; ++a) t.lo[a] = lo[(size_t)b * 3 + a];
    const int c = b * g.cells + cell_of_point(t, pts[(size_t)i * 3], pts[(size_t)i * 3 + 1], pts[(size_t)i * 3 + 2]);
    cell_of[i] = c;
    atomicAdd(pop + c, 1);
}

// launch "scatter", live row i of m: its Row into cell order
__device__ __forceinline__ void scatter_packed_row(const double* __restrict__ pts, int i, int m,
                                                   const int32_t* __restrict__ cell_of, int32_t* __restrict__ cursor,
                                                   Row* __restrict__ rows) {
    Row r;
    r.x = pts[(size_t)i * 3];
    r.y = pts[(size_t)i * 3 + 1];
    r.z = pts[(size_t)i * 3 + 2];
    r.pos = i;
    r.cell = cell_of[i];
    scatter_row(r, m, cursor, rows);
}

// ---- host.  The sort's four arrays in a workspace, behind `front` bytes of the caller's own (a multiple of 16)
inline size_t pad16(size_t v) { return (v + 15) / 16 * 16; }

struct SortLayout {
    size_t rows, cell_of, start, pop, bytes;
    int64_t cells;
};
// false where the shape is not served: total outside 1 .. max_total, or B * cells_per_tile outside 1 .. 2^22
inline bool sort_layout(int64_t total, int64_t max_total, int64_t B, int64_t cells_per_tile, size_t front, SortLayout& L) {
    if (total < 1 || total > max_total || B < 1 || cells_per_tile < 1 || B > kMaxCells || cells_per_tile > kMaxCells ||
        B * cells_per_tile > kMaxCells)
        return false;
    const size_t T = (size_t)total;
    L.cells = B * cells_per_tile;
    size_t at = front;
    L.rows = at, at += T * sizeof(Row);
    L.cell_of = at, at += pad16(T * 4);
    L.start = at, at += pad16(((size_t)L.cells + 1) * 4);
    L.pop = at, at += pad16((size_t)L.cells * 4);
    L.bytes = at;
    return true;
}

// The checks of a call's radius, dims and mult, in two steps because the calls refuse their other arguments in between
// (what is invalid before what is not served).  First the values that mean nothing ...
inline int grid_args_valid(const char* who, double radius, int dim_x, int dim_y, int dim_z, int64_t mult) {
    if (!(radius > 0.0) || !std::isfinite(radius))
        return sn::fail(SN_ERR_INVALID_ARG, "%s: radius must be positive and finite", who);
    if (dim_x < 1 || dim_y < 1 || dim_z < 1 || mult < 1)
        return sn::fail(SN_ERR_INVALID_ARG, "%s: dims and mult must be at least 1 (got %d, %d, %d; %lld)", who, dim_x, dim_y,
                        dim_z, (long long)mult);
    return SN_OK;
}
// ... then the cell budget and the range of radius, and the grid of one tile (its lo is read per tile on the device)
inline int grid_of_tiles(const char* who, double radius, int B, int dim_x, int dim_y, int dim_z, int64_t mult, CellGrid& g) {
    const int64_t cpt = (int64_t)dim_x * dim_y;   // (each factor < 2^31: no overflow before the checks)
    if (cpt > kMaxCells || cpt * dim_z > kMaxCells || cpt * dim_z * B > kMaxCells)
        return sn::fail(SN_ERR_UNSUPPORTED, "%s: more than 2^22 cells (B * dims = %d * %d * %d * %d)", who, B, dim_x, dim_y, dim_z);
    if (radius < kEpsMin || radius > kEpsMax)
        return sn::fail(SN_ERR_UNSUPPORTED, "%s: radius beyond what is served (1e-150 .. 1e150)", who);
    const double side = cell_side((double)mult, radius);
    if (!std::isfinite(side)) return sn::fail(SN_ERR_UNSUPPORTED, "%s: mult * radius is not finite", who);
    g.lo[0] = g.lo[1] = g.lo[2] = 0.0;
    g.inv = 1.0 / side;
    g.dim[0] = dim_x, g.dim[1] = dim_y, g.dim[2] = dim_z;
    g.cells = (int)(cpt * dim_z);   // per tile
    return SN_OK;
}

}  // namespace
