// K21 -- nearest neighbours: the k smallest neighbour distances of every point within a radius, the number of neighbours
// inside it, and per-tile spacing statistics (sn_knn_points, sn_knn_tile_stats).
// replaces: avg_dist_points (utils/pcd_processing.py:477-505: a Python loop over all pairs with np.linalg.norm, a list of
//           distances that is sorted again for every point), the reference's only question about a cloud's spacing; and is
//           what statistical / radius outlier removal and the k-distance curve for DBSCAN's eps are built on.
//
// Definition (normative, include/scenenet_hip.h): for row p of tile b a candidate is a row q != p (by row index) of the
// same tile with d2 = (dx*dx + dy*dy) + dz*dz <= radius*radius in fp64 in exactly this form (this file is built with
// -ffp-contract=off), the comparison literal; with SN_KNN_EXCLUDE_ZERO also d2 > 0.  found = all candidates; the k best by
// (d2, row index) ascending; mean_dist = the ascending sum of their square roots over their number.  Every result is a
// function of the candidate SET: the list is ordered by a total order on (d2, row), found is a count.
//
// The rows are counting-sorted into the cell grid of cell_grid.h, with eps = radius and k = mult, from each tile's own lo:
// the cell key is tile * cells_per_tile + local cell, so tiles never meet; a Row is (x, y, z, row index, key).  The sort is
// cell_grid.h's text (the bodies of launches 1 to 3, the layout of its arrays, the checks of the grid's arguments), which
// shape.hip runs too; the kernels are this file's, so that a trace tells the two calls apart.
//   1 cells    tile (binary search in offsets) and cell of every row, populations (integer atomics, zeroed by a small
//              launch in front); rows that no tile owns get their empty result here
//   2 prefix   cell_starts
//   3 scatter  scatter_row
//   4 search   one thread per row IN CELL ORDER: the 9 runs of the 27 cells, the k best in registers (compile-time K in
//              {1, 4, 8, 16}, insertion by an unrolled compare-and-shift: no runtime-indexed private array), results stored
//              at the row's own index
// statistics: per-chunk partials in row order (one workgroup per chunk of 256 rows of a tile, a fixed shuffle tree), then
// one combining pass per tile in chunk order -- no floating-point atomics, equal bits on every run.
//
// Bound: launch 4 by the latency of the candidate loads, as K10's launches 4, 5 and 8.
#include "common.h"
#include "cell_grid.h"
#include "packed_rows.h"
#include "scan.h"
#include <cmath>

namespace {

constexpr int kThreads = 256;
constexpr int kChunk = kThreads;        // rows per workgroup of launches 1, 3, 4 and per partial of the statistics
constexpr int kStatParts = 128;         // workgroups per tile of the partials kernel
constexpr int kMaxK = SN_KNN_MAX_K;

using sn::live_rows;   // packed_rows.h
using sn::pos_inf;
using sn::quiet_nan;

// ---- 0: the populations zeroed by a launch of this file, not by a memset node ("Launches")
__global__ __launch_bounds__(kThreads) void knn_zero_kernel(int32_t* __restrict__ pop, int cells) {
    zero_population(pop, cells, blockIdx.x * kThreads + threadIdx.x);
}

// ---- 1: the cell key of every row and the cells' populations; the empty result of rows outside every tile
__global__ __launch_bounds__(kThreads) void knn_cells_kernel(const double* __restrict__ pts,
                                                             const int64_t* __restrict__ offsets, int total, int B,
                                                             const double* __restrict__ lo, CellGrid g, int k,
                                                             int32_t* __restrict__ cell_of, int32_t* __restrict__ pop,
                                                             double* __restrict__ d2, int32_t* __restrict__ found,
                                                             double* __restrict__ mean_dist, int64_t* __restrict__ index) {
    const int m = live_rows(offsets, B, total);
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= total) return;
    if (i >= m) {
        for (int j = 0; j < k; ++j) {
            d2[(size_t)i * k + j] = pos_inf();
            if (index) index[(size_t)i * k + j] = -1;
        }
        found[i] = 0;
        if (mean_dist) mean_dist[i] = quiet_nan();
        return;
    }
    count_packed_row(pts, offsets, B, lo, g, i, cell_of, pop);
}

// ---- 2: one workgroup: the cells' starts and cursors
__global__ __launch_bounds__(kScanThreads) void knn_prefix_kernel(int32_t* __restrict__ pop, int cells,
                                                                  int32_t* __restrict__ start) {
    __shared__ int64_t s_wave[kScanThreads / 64];
    cell_starts(pop, cells, start, s_wave);
}

// ---- 3: rows into cell order
__global__ __launch_bounds__(kThreads) void knn_scatter_kernel(const double* __restrict__ pts,
                                                               const int64_t* __restrict__ offsets, int total, int B,
                                                               const int32_t* __restrict__ cell_of,
                                                               int32_t* __restrict__ cursor, Row* __restrict__ rows) {
    const int m = live_rows(offsets, B, total);
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i < m) scatter_packed_row(pts, i, m, cell_of, cursor, rows);
}

// ---- 4: the search.  (v, p) sorts in front of (d, i) iff v < d, or v == d and p < i
__device__ __forceinline__ bool in_front(double v, int p, double d, int i) { return v < d || (v == d && p < i); }

template <int K>
struct Best {
    double d[K];
    int id[K];
    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int j = 0; j < K; ++j) d[j] = pos_inf(), id[j] = 0x7fffffff;
    }
    // compile-time indices only: slot j takes its left neighbour where the newcomer sorts in front of that one, the
    // newcomer where it sorts in front of slot j alone, and keeps its own otherwise
    __device__ __forceinline__ void insert(double v, int p) {
        if (!in_front(v, p, d[K - 1], id[K - 1])) return;
        bool before[K];
#pragma unroll
        for (int j = 0; j < K; ++j) before[j] = in_front(v, p, d[j], id[j]);
#pragma unroll
        for (int j = K - 1; j > 0; --j) {
            d[j] = before[j - 1] ? d[j - 1] : (before[j] ? v : d[j]);
            id[j] = before[j - 1] ? id[j - 1] : (before[j] ? p : id[j]);
        }
        if (before[0]) d[0] = v, id[0] = p;
    }
};

template <int K>
__global__ __launch_bounds__(kThreads) void knn_search_kernel(const int64_t* __restrict__ offsets, int total, int B,
                                                              CellGrid g, double r2, int k, int exclude_zero,
                                                              const int32_t* __restrict__ start,
                                                              const Row* __restrict__ rows, double* __restrict__ d2_out,
                                                              int32_t* __restrict__ found_out,
                                                              double* __restrict__ mean_out,
                                                              int64_t* __restrict__ index_out) {
#pragma clang fp contract(off)
    const int m = live_rows(offsets, B, total);
    const int r = blockIdx.x * kThreads + threadIdx.x;
    if (r >= m) return;
    const Row me = rows[r];
    if ((unsigned)me.cell >= (unsigned)(B * g.cells)) return;   // (never, behind launches 1 to 3 of the same call)
    Best<K> best;
    best.clear();
    int found = 0;
    const int tile = me.cell / g.cells, local = me.cell - tile * g.cells;
    // the 9 runs of for_candidates (cell_grid.h) on the tile's slice of start, in a loop of the kernel's own
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
                if (!(d2 <= r2) || q.pos == me.pos || (exclude_zero && !(d2 > 0.0))) continue;
                ++found;
                best.insert(d2, q.pos);
            }
        }
    if ((unsigned)me.pos >= (unsigned)total) return;
    const size_t o = (size_t)me.pos * k;
    const int c = found < k ? found : k;
    double sum = 0.0;
#pragma unroll
    for (int j = 0; j < K; ++j) {
        if (j < k) {
            d2_out[o + j] = best.d[j];   // (+inf beyond the candidates)
            if (index_out) index_out[o + j] = j < c ? (int64_t)best.id[j] : (int64_t)-1;
            if (j < c) {
                const double s = sqrt(best.d[j]);
                sum = j == 0 ? s : sum + s;
            }
        }
    }
    found_out[me.pos] = found;
    if (mean_out) mean_out[me.pos] = c > 0 ? sum / (double)c : quiet_nan();
}

// ---- statistics.  A partial: n_valid, n_full (integers as bit patterns), sum, sum_sq, max
constexpr int kStat = SN_KNN_NSTAT;

// tile b's chunk j sits at slot offsets[b] / kChunk + b + j: the slots of two tiles never overlap, as
// floor(o / c) + ceil(n / c) <= floor((o + n) / c) + 1
__device__ __forceinline__ int64_t partial_slot(int64_t off, int b, int j) { return off / kChunk + b + j; }

__global__ __launch_bounds__(kThreads) void knn_stat_partials_kernel(const double* __restrict__ mean_dist,
                                                                     const int32_t* __restrict__ found,
                                                                     const int64_t* __restrict__ offsets, int64_t total,
                                                                     int k, double* __restrict__ partials,
                                                                     int64_t n_slots) {
#pragma clang fp contract(off)
    __shared__ double s_sum[kThreads / 64], s_sq[kThreads / 64], s_max[kThreads / 64];
    __shared__ int s_valid[kThreads / 64], s_full[kThreads / 64];
    const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int64_t first = offsets[b], end = offsets[b + 1];
    first = first < 0 ? 0 : first;
    end = end > total ? total : end;
    const int64_t n = end - first;
    const int chunks = n <= 0 ? 0 : (int)((n + kChunk - 1) / kChunk);
    for (int j = blockIdx.x; j < chunks; j += kStatParts) {
        const int64_t i = first + (int64_t)j * kChunk + threadIdx.x;
        int valid = 0, full = 0;
        double v = 0.0, sq = 0.0, mx = -pos_inf();
        if (i < end) {
            const int f = found[i];
            if (f >= 1) {
                valid = 1;
                full = f >= k ? 1 : 0;
                v = mean_dist[i];
                sq = v * v;
                mx = v;
            }
        }
        // a fixed tree: lanes by xor-shuffles (both sides form the same sum, addition commutes), then the waves in order
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            valid += __shfl_xor(valid, off, 64);
            full += __shfl_xor(full, off, 64);
            v = v + __shfl_xor(v, off, 64);
            sq = sq + __shfl_xor(sq, off, 64);
            const double o = __shfl_xor(mx, off, 64);
            mx = o > mx ? o : mx;
        }
        if (lane == 0) s_valid[wave] = valid, s_full[wave] = full, s_sum[wave] = v, s_sq[wave] = sq, s_max[wave] = mx;
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int w = 1; w < kThreads / 64; ++w) {
                valid += s_valid[w], full += s_full[w];
                v = v + s_sum[w];
                sq = sq + s_sq[w];
                mx = s_max[w] > mx ? s_max[w] : mx;
            }
            const int64_t slot = partial_slot(first, b, j);
            if ((uint64_t)slot < (uint64_t)n_slots) {
                double* p = partials + slot * kStat;
                p[0] = __longlong_as_double((long long)valid);
                p[1] = __longlong_as_double((long long)full);
                p[2] = v, p[3] = sq, p[4] = mx;
            }
        }
        __syncthreads();
    }
}

// one workgroup per tile: thread t sums its run of consecutive chunks in chunk order, thread 0 the threads' sums in
// thread order -- the chunks of a tile in ascending order under one fixed bracketing
__global__ __launch_bounds__(kThreads) void knn_stat_combine_kernel(const int64_t* __restrict__ offsets, int64_t total,
                                                                    const double* __restrict__ partials, int64_t n_slots,
                                                                    double* __restrict__ stats) {
#pragma clang fp contract(off)
    __shared__ double s_sum[kThreads], s_sq[kThreads], s_max[kThreads];
    __shared__ long long s_valid[kThreads], s_full[kThreads];
    const int b = blockIdx.x;
    int64_t first = offsets[b], end = offsets[b + 1];
    first = first < 0 ? 0 : first;
    end = end > total ? total : end;
    const int64_t n = end - first;
    const int chunks = n <= 0 ? 0 : (int)((n + kChunk - 1) / kChunk);
    const int per = (chunks + kThreads - 1) / kThreads;
    long long valid = 0, full = 0;
    double v = 0.0, sq = 0.0, mx = -pos_inf();
    for (int q = 0; q < per; ++q) {
        const int j = threadIdx.x * per + q;
        const int64_t slot = partial_slot(first, b, j);
        if (j < chunks && (uint64_t)slot < (uint64_t)n_slots) {
            const double* p = partials + slot * kStat;
            valid += __double_as_longlong(p[0]);
            full += __double_as_longlong(p[1]);
            v = v + p[2];
            sq = sq + p[3];
            mx = p[4] > mx ? p[4] : mx;
        }
    }
    s_valid[threadIdx.x] = valid, s_full[threadIdx.x] = full;
    s_sum[threadIdx.x] = v, s_sq[threadIdx.x] = sq, s_max[threadIdx.x] = mx;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kThreads; ++w) {
            valid += s_valid[w], full += s_full[w];
            v = v + s_sum[w];
            sq = sq + s_sq[w];
            mx = s_max[w] > mx ? s_max[w] : mx;
        }
        double* o = stats + (size_t)b * kStat;
        o[0] = (double)valid, o[1] = (double)full, o[2] = v, o[3] = sq, o[4] = mx;
    }
}

// ------------------------------------------------------------------------------------------------------------------ host
// the statistics partials lead the workspace, the sort's arrays (cell_grid.h) behind them: sn_knn_tile_stats finds its
// slots without the grid
int64_t stat_slots(int64_t total, int64_t B) { return total / kChunk + B + 1; }
size_t partials_bytes(int64_t total, int64_t B) { return pad16((size_t)stat_slots(total, B) * kStat * 8); }
bool layout_of(int64_t total, int64_t B, int64_t cells_per_tile, SortLayout& L) {
    return sort_layout(total, ((int64_t)1 << 31) - 1, B, cells_per_tile, partials_bytes(total, B), L);
}

template <int K>
void launch_search(dim3 grid, hipStream_t s, const int64_t* offsets, int total, int B, const CellGrid& g, double r2, int k,
                   int exclude_zero, const int32_t* start, const Row* rows, double* d2, int32_t* found, double* mean_dist,
                   int64_t* index) {
    hipLaunchKernelGGL(knn_search_kernel<K>, grid, dim3(kThreads), 0, s, offsets, total, B, g, r2, k, exclude_zero, start, rows,
                       d2, found, mean_dist, index);
}

int run(const double* pts, const int64_t* offsets, int64_t total, int B, double radius, int k, int flags, const double* lo,
        int dim_x, int dim_y, int dim_z, int64_t mult, void* ws, size_t ws_bytes, double* d2, int32_t* found,
        double* mean_dist, int64_t* index, int first, int last, sn_stream_t stream) {
    const char* who = "sn_knn_points";
    if (!pts || !offsets || !lo || !ws || !d2 || !found)
        return sn::fail(SN_ERR_INVALID_ARG, "%s: null pointer (pts, offsets, lo, ws, d2, found)", who);
    if (total <= 0) return sn::fail(SN_ERR_INVALID_ARG, "%s: total must be positive (got %lld)", who, (long long)total);
    if (B <= 0) return sn::fail(SN_ERR_INVALID_ARG, "%s: B must be positive (got %d)", who, B);
    if (k < 1) return sn::fail(SN_ERR_INVALID_ARG, "%s: k must be at least 1 (got %d)", who, k);
    if (int e = grid_args_valid(who, radius, dim_x, dim_y, dim_z, mult)) return e;
    if (flags & ~SN_KNN_EXCLUDE_ZERO) return sn::fail(SN_ERR_INVALID_ARG, "%s: unknown flags %d", who, flags);
    if (k > kMaxK) return sn::fail(SN_ERR_UNSUPPORTED, "%s: k beyond what is served (at most %d, got %d)", who, kMaxK, k);
    if (total >= ((int64_t)1 << 31)) return sn::fail(SN_ERR_UNSUPPORTED, "%s: total < 2^31 rows are served", who);
    CellGrid g;
    if (int e = grid_of_tiles(who, radius, B, dim_x, dim_y, dim_z, mult, g)) return e;
    if ((uintptr_t)pts % 8 || (uintptr_t)offsets % 8 || (uintptr_t)lo % 8 || (uintptr_t)ws % 16 || (uintptr_t)d2 % 8 ||
        (uintptr_t)found % 4 || (uintptr_t)mean_dist % 8 || (uintptr_t)index % 8)
        return sn::fail(SN_ERR_INVALID_ARG, "%s: pts / offsets / lo / d2 / mean_dist / index must be 8-byte aligned, ws "
                        "16-byte, found 4-byte", who);
    SortLayout L;
    layout_of(total, B, g.cells, L);
    if (ws_bytes < L.bytes)
        return sn::fail(SN_ERR_INVALID_ARG, "%s: ws holds %zu bytes, %zu needed (sn_knn_ws_bytes)", who, ws_bytes, L.bytes);

    hipStream_t s = sn::as_stream(stream);
    char* w = static_cast<char*>(ws);
    Row* rows = reinterpret_cast<Row*>(w + L.rows);
    int32_t* cell_of = reinterpret_cast<int32_t*>(w + L.cell_of);
    int32_t* start = reinterpret_cast<int32_t*>(w + L.start);
    int32_t* pop = reinterpret_cast<int32_t*>(w + L.pop);
    const int n = (int)total;
    const dim3 grid((unsigned)((n + kThreads - 1) / kThreads)), block(kThreads);
    const double r2 = radius * radius;
    const int ez = (flags & SN_KNN_EXCLUDE_ZERO) ? 1 : 0;

    if (first <= 1 && last >= 1) {
        hipLaunchKernelGGL(knn_zero_kernel, dim3((unsigned)((L.cells + kThreads - 1) / kThreads)), block, 0, s, pop,
                           (int)L.cells);
        hipLaunchKernelGGL(knn_cells_kernel, grid, block, 0, s, pts, offsets, n, B, lo, g, k, cell_of, pop, d2, found, mean_dist,
                           index);
        if (int e = sn::check_launch("sn_knn_points(cells)")) return e;
    }
    if (first <= 2 && last >= 2) {
        hipLaunchKernelGGL(knn_prefix_kernel, dim3(1), dim3(kScanThreads), 0, s, pop, (int)L.cells, start);
        if (int e = sn::check_launch("sn_knn_points(prefix)")) return e;
    }
    if (first <= 3 && last >= 3) {
        hipLaunchKernelGGL(knn_scatter_kernel, grid, block, 0, s, pts, offsets, n, B, cell_of, pop, rows);
        if (int e = sn::check_launch("sn_knn_points(scatter)")) return e;
    }
    if (first <= 4 && last >= 4) {
        // the requested k rounded up to the next instantiation; the first k columns are stored
        if (k <= 1) launch_search<1>(grid, s, offsets, n, B, g, r2, k, ez, start, rows, d2, found, mean_dist, index);
        else if (k <= 4) launch_search<4>(grid, s, offsets, n, B, g, r2, k, ez, start, rows, d2, found, mean_dist, index);
        else if (k <= 8) launch_search<8>(grid, s, offsets, n, B, g, r2, k, ez, start, rows, d2, found, mean_dist, index);
        else launch_search<16>(grid, s, offsets, n, B, g, r2, k, ez, start, rows, d2, found, mean_dist, index);
        if (int e = sn::check_launch("sn_knn_points(search)")) return e;
    }
    return SN_OK;
}

}  // namespace

extern "C" int sn_knn_chunk_points(void) { return kChunk; }

extern "C" size_t sn_knn_ws_bytes(int64_t total, int B, int64_t cells_per_tile) {
    SortLayout L;
    return layout_of(total, B, cells_per_tile, L) ? L.bytes : 0;
}

extern "C" int sn_knn_points(const double* pts, const int64_t* offsets, int64_t total, int B, double radius, int k, int flags,
                             const double* lo, int dim_x, int dim_y, int dim_z, int64_t mult, void* ws, size_t ws_bytes,
                             double* d2, int32_t* found, double* mean_dist, int64_t* index, sn_stream_t stream) {
    return run(pts, offsets, total, B, radius, k, flags, lo, dim_x, dim_y, dim_z, mult, ws, ws_bytes, d2, found, mean_dist, index,
               1, SN_KNN_LAUNCHES, stream);
}

extern "C" int sn_knn_points_launches(const double* pts, const int64_t* offsets, int64_t total, int B, double radius, int k,
                                      int flags, const double* lo, int dim_x, int dim_y, int dim_z, int64_t mult, void* ws,
                                      size_t ws_bytes, double* d2, int32_t* found, double* mean_dist, int64_t* index, int first,
                                      int last, sn_stream_t stream) {
    if (first < 1 || last > SN_KNN_LAUNCHES || first > last)
        return sn::fail(SN_ERR_INVALID_ARG, "sn_knn_points_launches: 1 <= first <= last <= %d", SN_KNN_LAUNCHES);
    return run(pts, offsets, total, B, radius, k, flags, lo, dim_x, dim_y, dim_z, mult, ws, ws_bytes, d2, found, mean_dist, index,
               first, last, stream);
}

extern "C" int sn_knn_tile_stats(const double* mean_dist, const int32_t* found, const int64_t* offsets, int64_t total, int B,
                                 int k, void* ws, size_t ws_bytes, double* stats, sn_stream_t stream) {
    const char* who = "sn_knn_tile_stats";
    if (!mean_dist || !found || !offsets || !ws || !stats)
        return sn::fail(SN_ERR_INVALID_ARG, "%s: null pointer (mean_dist, found, offsets, ws, stats)", who);
    if (total <= 0) return sn::fail(SN_ERR_INVALID_ARG, "%s: total must be positive (got %lld)", who, (long long)total);
    if (B <= 0) return sn::fail(SN_ERR_INVALID_ARG, "%s: B must be positive (got %d)", who, B);
    if (k < 1) return sn::fail(SN_ERR_INVALID_ARG, "%s: k must be at least 1 (got %d)", who, k);
    if (k > kMaxK) return sn::fail(SN_ERR_UNSUPPORTED, "%s: k beyond what is served (at most %d, got %d)", who, kMaxK, k);
    if (total >= ((int64_t)1 << 31) || B > 65535)
        return sn::fail(SN_ERR_UNSUPPORTED, "%s: total < 2^31 rows and B <= 65535 tiles are served", who);
    if ((uintptr_t)mean_dist % 8 || (uintptr_t)found % 4 || (uintptr_t)offsets % 8 || (uintptr_t)ws % 16 || (uintptr_t)stats % 8)
        return sn::fail(SN_ERR_INVALID_ARG, "%s: mean_dist / offsets / stats must be 8-byte aligned, ws 16-byte, found 4-byte",
                        who);
    const size_t need = partials_bytes(total, B);   // (the partials lead the workspace whatever the grid is)
    const int64_t n_slots = stat_slots(total, B);
    if (ws_bytes < need)
        return sn::fail(SN_ERR_INVALID_ARG, "%s: ws holds %zu bytes, %zu needed (sn_knn_ws_bytes)", who, ws_bytes, need);
    hipStream_t s = sn::as_stream(stream);
    double* partials = static_cast<double*>(ws);
    hipLaunchKernelGGL(knn_stat_partials_kernel, dim3(kStatParts, (unsigned)B), dim3(kThreads), 0, s, mean_dist, found, offsets,
                       total, k, partials, n_slots);
    if (int e = sn::check_launch("sn_knn_tile_stats(partials)")) return e;
    hipLaunchKernelGGL(knn_stat_combine_kernel, dim3((unsigned)B), dim3(kThreads), 0, s, offsets, total, partials, n_slots,
                       stats);
    return sn::check_launch("sn_knn_tile_stats(combine)");
}
