// The cell grid of the neighbourhood kernels, shared by dbscan.hip (K10) and knn.hip (K21): cubic cells of side
// k * eps * (1 + 2^-20), points binned by axis_cell (monotone, clamped), so that two points within eps of each other never
// sit two cells apart and the 27 cells around a point's own hold every neighbour.  One rule, one proof, one text.
//
// The grid is an accelerator only.  Points are counting-sorted into cell order as rows (x, y, z, position, cell): the
// populations per cell (integer atomics, the files' own launch 1), their exclusive prefix and the cursors (cell_starts, one
// workgroup), the rows stored where the cursors say (scatter_row).  With z the fastest cell axis the three cells of one
// (x, y) column are ONE contiguous run of rows: 9 runs per home point (for_candidates).  The order of rows inside a cell depends
// on scheduling (an integer cursor); every result is a count, a minimum, a set union or a function of the candidate SET
// over the runs, so none does.  Device text and one host helper, no kernels: a trace keeps telling K10's launches from K21's.
#pragma once
#include "scan.h"
#include <hip/hip_runtime.h>

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

}  // namespace
