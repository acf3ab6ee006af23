// K1's binning of a point into a tile's edge tables, shared by voxel.hip (K1) and thin.hip (K17): one rule, one text.
#pragma once
#include <hip/hip_runtime.h>
#include <cfloat>

namespace sn {

// ---------------------------------------------------------------- binning
// largest j with e[j] < p  (== numpy.searchsorted(e, p, side='left') - 1), in [-1, n].  bin_guess is the arithmetic
// estimate (right except for points sitting on an edge and last-bit rounding), bin_search walks from any start to the
// exact answer with dependent LDS reads; Binner::flat confirms the three guesses with one round of independent reads
// and only walks when a guess fails.
// The guess is clamped to [0, n-1] so that e[k] and e[k+1] both exist: the confirmation then needs no special cases.
__device__ __forceinline__ int bin_guess(double p, int n, double lo, double inv_step) {
    const int g = (int)((p - lo) * inv_step);   // v_cvt_i32_f64 saturates; NaN -> 0
    return max(0, min(g, n - 1));
}
__device__ __forceinline__ int bin_search(double p, const double* e, int n, int k) {
    while (k < n && e[k + 1] < p) ++k;
    while (k >= 0 && !(e[k] < p)) --k;
    return k;
}

struct Binner {
    const double *ex, *ey, *ez;
    double lo[3], inv[3];
    int nx, ny, nz;

    // edges must already sit in LDS at `edges`; d = this tile's descriptor
    __device__ __forceinline__ void init(const double* edges, const double* d, int nx_, int ny_, int nz_) {
        ex = edges; ey = edges + nx_ + 1; ez = edges + nx_ + ny_ + 2;
        nx = nx_; ny = ny_; nz = nz_;
        // the guess only needs the bin width: the first step of each edge table (== (hi - lo) / n up to rounding, and
        // right for the padded per-tile tables of the size mode, whose real n is not the table's)
        const double* e[3] = {ex, ey, ez};
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            lo[a] = d[a];
            const double step = e[a][1] - e[a][0];
            inv[a] = (step > 0.0 && step < DBL_MAX) ? 1.0 / step : 0.0;
        }
    }
    // flat [z][x][y] index, or -1 when the point is NaN / outside the edge table (np.clip to n).
    // Fast path, branch-free: three clamped guesses, six independent LDS reads, six compares -- a guess k stands iff
    // e[k] < p and not e[k+1] < p, exactly where bin_search(k) would stop.  Everything else (a point sitting on an
    // edge, the tile's minimum, NaN, a point beyond the table) takes the exact walk; a wave skips that branch as a
    // whole when none of its points needs it ([measured] the first form, with its per-axis special cases, spent
    // ~100 VALU instructions per point).
    __device__ __forceinline__ int flat(double x, double y, double z) const {
        int ix = bin_guess(x, nx, lo[0], inv[0]);
        int iy = bin_guess(y, ny, lo[1], inv[1]);
        int iz = bin_guess(z, nz, lo[2], inv[2]);
        const double x0 = ex[ix], x1 = ex[ix + 1], y0 = ey[iy], y1 = ey[iy + 1], z0 = ez[iz], z1 = ez[iz + 1];
        const bool ok = (x0 < x) & !(x1 < x) & (y0 < y) & !(y1 < y) & (z0 < z) & !(z1 < z);
        if (!ok) {
            if (x != x || y != y || z != z) return -1;
            ix = max(bin_search(x, ex, nx, ix), 0);
            iy = max(bin_search(y, ey, ny, iy), 0);
            iz = max(bin_search(z, ez, nz, iz), 0);
            if (ix >= nx || iy >= ny || iz >= nz) return -1;
        }
        return (iz * nx + ix) * ny + iy;
    }
};

__device__ __forceinline__ void load_edges(double* edges, const double* d, int ne, int nthreads) {
    for (int i = threadIdx.x; i < ne; i += nthreads) edges[i] = d[6 + i];
    __syncthreads();
}

}  // namespace sn
