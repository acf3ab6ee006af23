// The cell grid of the neighbourhood kernels, shared by dbscan.hip (K10) and knn.hip (K21): cubic cells of side
// k * eps * (1 + 2^-20), points binned by axis_cell (monotone, clamped), so that two points within eps of each other never
// sit two cells apart and the 27 cells around a point's own hold every neighbour.  One rule, one proof, one text.
#pragma once
#include <hip/hip_runtime.h>

namespace {

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

}  // namespace
