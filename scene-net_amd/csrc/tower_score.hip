// K11 -- tower scores: K8's statistics rows filtered, merged and matched against the ground truth's towers
// (sn_tower_centroids, sn_tower_match).
// replaces: filter_towers, aggregate_centroids and the matching loop of compute_euc_dists (utils/observer_utils.py:413-549)
// as get_tower_proposals (:556-582) chains them: numpy on the host, one tile at a time, behind a copy of the tile's voxels.
//
// Everything these steps read sits in the [K, 12] integer rows sn_tower_proposals leaves per tile, so a tile is a few
// microseconds of work for ONE workgroup: the rows are strided over its lanes, the tile's planar rows live in LDS
// (<= 1024 rows x 16 B) and every O(K^2) step -- the pair tests, the means, the ranks-by-counting that stand in for
// np.unique's sort, the argmin -- reads them from there (every lane reads the same row j: an LDS broadcast).
//   centroids  1 launch, a workgroup per tile: coordinates + filter -> means -> first occurrences -> ranks -> agg
//   match      1 launch, a workgroup per tile: argmin per ground-truth row, the tile's counts added to `totals` with
//              64-bit integer atomics (one lane per tile)
//   dist sum   1 launch of one workgroup (only with totals): the hits' distances summed per tile in row order by one thread
//              each, then over the tiles in a fixed shape (strided runs, an LDS tree): no fp atomics, so identical bits
//              for identical inputs whatever the scheduling
// No workgroup waits for another.  All fp64 arithmetic is written in the header's order and rounded once per operation
// (this file is built with -ffp-contract=off); sqrt is the correctly rounded one.
//
// Bound: launch latency.  The data of a tile is K * 96 bytes.
#include "common.h"
#include "packed_rows.h"
#include <cmath>

namespace {

using sn::quiet_nan;   // packed_rows.h: the bit pattern K21 and K22 store too

constexpr int kThreads = 256;
constexpr int kSumThreads = 1024;
constexpr int kMaxRows = SN_TSCORE_MAX_ROWS;
constexpr int kMaxTiles = 65535;

struct Geom {
    double s[3];     // voxel size per grid axis
    double ctr[3];   // the filter's centre, scaled units
    int h, p0, p1;   // height axis and the two planar axes, ascending
};

// v[a] by selects: a run-time index into a kernel argument would go through scratch
__device__ __forceinline__ double pick(const double (&v)[3], int a) { return a == 0 ? v[0] : (a == 1 ? v[1] : v[2]); }

// the planar row of statistics row r (n_voxels > 0), by the header's coordinate rule
__device__ __forceinline__ void planar_of(const long long* r, const Geom& g, double& q0, double& q1) {
    const double n = (double)r[0];
    q0 = ((double)r[2 + g.p0] / n) * pick(g.s, g.p0);
    q1 = ((double)r[2 + g.p1] / n) * pick(g.s, g.p1);
}

__device__ __forceinline__ double extent_of(const long long* r, const Geom& g, int a) {
    const double s = pick(g.s, a);
    return (double)r[8 + a] * s - (double)r[5 + a] * s;
}

__device__ __forceinline__ int rows_of(int n_towers, int K) {   // the rows that can be present
    return n_towers < 0 ? 0 : (n_towers < K ? n_towers : K);
}

// ---- centroids: one workgroup per tile
__global__ __launch_bounds__(kThreads) void tscore_centroids_kernel(const long long* __restrict__ stats,
                                                                    const int32_t* __restrict__ n_towers, int K, Geom g,
                                                                    int apply_filter, double threshold, double tower_height,
                                                                    double rim_sq, double min_euc, uint8_t* __restrict__ keep,
                                                                    double* __restrict__ planar, double* __restrict__ agg,
                                                                    int32_t* __restrict__ n_agg, int32_t* __restrict__ status) {
    __shared__ double q[kMaxRows][2];      // planar rows (kept rows only are read)
    __shared__ double mean[kMaxRows][2];
    __shared__ uint8_t kept[kMaxRows];
    __shared__ uint8_t first[kMaxRows];    // kept, and no kept row in front of it has the same mean
    __shared__ int n_first;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int nt = n_towers[b];
    const int n = rows_of(nt, K);
    const long long* rows = stats + (size_t)b * K * SN_TOWER_NSTAT;
    if (tid == 0) n_first = 0;

    // coordinates and the filter
    for (int i = tid; i < K; i += kThreads) {
        bool k = false;
        double q0 = quiet_nan(), q1 = quiet_nan();
        if (i < n) {
            const long long* r = rows + (size_t)i * SN_TOWER_NSTAT;
            if (r[0] > 0) {
                planar_of(r, g, q0, q1);
                k = true;
                if (apply_filter) {
                    const double eh = extent_of(r, g, g.h), e0 = extent_of(r, g, g.p0), e1 = extent_of(r, g, g.p1);
                    const double spread = e0 > e1 ? e0 : e1;
                    const double dx = q0 - pick(g.ctr, g.p0), dy = q1 - pick(g.ctr, g.p1);
                    k = ((eh >= tower_height) || (spread <= threshold)) && (dx * dx + dy * dy <= rim_sq);
                }
            }
        }
        kept[i] = k;
        q[i][0] = q0;
        q[i][1] = q1;
        keep[(size_t)b * K + i] = k ? 1 : 0;
        if (planar) {
            planar[((size_t)b * K + i) * 2 + 0] = q0;
            planar[((size_t)b * K + i) * 2 + 1] = q1;
        }
    }
    __syncthreads();

    // mean_i over the kept j within min_euc, added in ascending j from 0.0
    for (int i = tid; i < n; i += kThreads) {
        if (!kept[i]) continue;
        const double x = q[i][0], y = q[i][1];
        double s0 = 0.0, s1 = 0.0;
        int cnt = 0;
        for (int j = 0; j < n; ++j) {
            if (!kept[j]) continue;
            const double dx = q[j][0] - x, dy = q[j][1] - y;
            if (sqrt(dx * dx + dy * dy) <= min_euc) {
                s0 = s0 + q[j][0];
                s1 = s1 + q[j][1];
                ++cnt;
            }
        }
        mean[i][0] = s0 / (double)cnt;    // cnt >= 1: the row itself
        mean[i][1] = s1 / (double)cnt;
    }
    __syncthreads();

    // first occurrences of each distinct mean
    int mine = 0;
    for (int i = tid; i < K; i += kThreads) {
        bool f = i < n && kept[i];
        if (f) {
            const double x = mean[i][0], y = mean[i][1];
            for (int j = 0; j < i; ++j)
                if (kept[j] && mean[j][0] == x && mean[j][1] == y) {
                    f = false;
                    break;
                }
        }
        first[i] = f;
        mine += f;
    }
    if (mine) atomicAdd(&n_first, mine);
    __syncthreads();

    // rank by counting: the distinct means that sort in front (column 0, then column 1)
    for (int i = tid; i < n; i += kThreads) {
        if (!first[i]) continue;
        const double x = mean[i][0], y = mean[i][1];
        int rank = 0;
        for (int j = 0; j < n; ++j)
            if (first[j] && (mean[j][0] < x || (mean[j][0] == x && mean[j][1] < y))) ++rank;
        agg[((size_t)b * K + rank) * 2 + 0] = x;     // rank < n_first <= K: distinct rows have distinct ranks
        agg[((size_t)b * K + rank) * 2 + 1] = y;
    }
    const int M = n_first;
    for (int i = M + tid; i < K; i += kThreads) {
        agg[((size_t)b * K + i) * 2 + 0] = quiet_nan();
        agg[((size_t)b * K + i) * 2 + 1] = quiet_nan();
    }
    if (tid == 0) {
        n_agg[b] = M;
        status[b] = nt > K ? 1 : 0;
    }
}

// ---- match: one workgroup per tile
__global__ __launch_bounds__(kThreads) void tscore_match_kernel(const double* __restrict__ agg, const int32_t* __restrict__ n_agg,
                                                                const int32_t* __restrict__ status_pred, int Kp,
                                                                const long long* __restrict__ gt_stats,
                                                                const int32_t* __restrict__ gt_n_towers, int Kg, Geom g,
                                                                double hit_dist, int32_t* __restrict__ match,
                                                                double* __restrict__ dist, double* __restrict__ gt_planar,
                                                                unsigned long long* __restrict__ totals) {
    __shared__ double a[kMaxRows][2];
    __shared__ uint8_t used[kMaxRows];     // the row is the match of a hit
    __shared__ int counts[3];              // gt rows, hits, unused aggregated rows
    const int b = blockIdx.x, tid = threadIdx.x;
    int M = n_agg[b];
    M = M < 0 ? 0 : (M < Kp ? M : Kp);
    const int gnt = gt_n_towers[b];
    const int n = rows_of(gnt, Kg);
    const long long* rows = gt_stats + (size_t)b * Kg * SN_TOWER_NSTAT;
    for (int m = tid; m < M; m += kThreads) {
        a[m][0] = agg[((size_t)b * Kp + m) * 2 + 0];
        a[m][1] = agg[((size_t)b * Kp + m) * 2 + 1];
        used[m] = 0;
    }
    if (tid < 3) counts[tid] = 0;
    __syncthreads();

    int n_gt = 0, n_hit = 0;
    for (int k = tid; k < Kg; k += kThreads) {
        int32_t best = -1;
        double d_best = quiet_nan(), g0 = quiet_nan(), g1 = quiet_nan();
        if (k < n) {
            const long long* r = rows + (size_t)k * SN_TOWER_NSTAT;
            if (r[0] > 0) {
                ++n_gt;
                planar_of(r, g, g0, g1);
                d_best = 0.0;
                for (int m = 0; m < M; ++m) {
                    const double dx = g0 - a[m][0], dy = g1 - a[m][1];
                    const double d = sqrt(dx * dx + dy * dy);
                    if (m == 0 || d < d_best) {     // the first of the smallest
                        d_best = d;
                        best = m;
                    }
                }
                if (best >= 0 && d_best <= hit_dist) {
                    ++n_hit;
                    used[best] = 1;                 // (several rows may store the same 1)
                }
            }
        }
        match[(size_t)b * Kg + k] = best;
        dist[(size_t)b * Kg + k] = d_best;
        if (gt_planar) {
            gt_planar[((size_t)b * Kg + k) * 2 + 0] = g0;
            gt_planar[((size_t)b * Kg + k) * 2 + 1] = g1;
        }
    }
    if (!totals) return;
    __syncthreads();
    int n_free = 0;
    for (int m = tid; m < M; m += kThreads) n_free += used[m] ? 0 : 1;
    if (n_gt) atomicAdd(&counts[0], n_gt);
    if (n_hit) atomicAdd(&counts[1], n_hit);
    if (n_free) atomicAdd(&counts[2], n_free);
    __syncthreads();
    if (tid == 0) {
        if ((status_pred[b] & 1) || gnt > Kg) {
            atomicAdd(totals + 1, 1ull);
        } else {
            atomicAdd(totals + 0, 1ull);
            atomicAdd(totals + 2, (unsigned long long)counts[0]);
            atomicAdd(totals + 3, (unsigned long long)M);
            atomicAdd(totals + 4, (unsigned long long)counts[1]);
            atomicAdd(totals + 5, (unsigned long long)(counts[0] - counts[1]));
            atomicAdd(totals + 6, (unsigned long long)counts[2]);
        }
    }
}

// ---- dist sum: one workgroup.  Thread t owns the tiles t, t + 1024, ...: each tile's hits in row order, the tiles one after
// another, then a tree over the 1024 threads -- a shape that depends on B and Kg alone.
__global__ __launch_bounds__(kSumThreads) void tscore_dist_sum_kernel(const int32_t* __restrict__ match,
                                                                      const double* __restrict__ dist,
                                                                      const int32_t* __restrict__ status_pred,
                                                                      const int32_t* __restrict__ gt_n_towers, int B, int Kg,
                                                                      double hit_dist, double* __restrict__ dist_total) {
    __shared__ double part[kSumThreads];
    const int tid = threadIdx.x;
    double acc = 0.0;
    for (int b = tid; b < B; b += kSumThreads) {
        if ((status_pred[b] & 1) || gt_n_towers[b] > Kg) continue;   // a skipped tile
        double tile = 0.0;
        for (int k = 0; k < Kg; ++k) {
            const double d = dist[(size_t)b * Kg + k];
            if (match[(size_t)b * Kg + k] >= 0 && d <= hit_dist) tile = tile + d;
        }
        acc = acc + tile;
    }
    part[tid] = acc;
    __syncthreads();
    for (int off = kSumThreads / 2; off > 0; off >>= 1) {
        if (tid < off) part[tid] = part[tid] + part[tid + off];
        __syncthreads();
    }
    if (tid == 0) *dist_total = *dist_total + part[0];
}

// ------------------------------------------------------------------------------------------------------------------ host
int geom_of(const char* who, int height_axis, const double* voxel_size_host, const double* center_host, Geom& g) {
    if (height_axis < 0 || height_axis > 2) return sn::fail(SN_ERR_INVALID_ARG, "%s: height_axis must be 0, 1 or 2", who);
    for (int k = 0; k < 3; ++k) {
        g.s[k] = voxel_size_host ? voxel_size_host[k] : 1.0;
        if (!(g.s[k] > 0.0) || !std::isfinite(g.s[k]))
            return sn::fail(SN_ERR_INVALID_ARG, "%s: voxel_size must be positive and finite", who);
        g.ctr[k] = center_host ? center_host[k] : 0.0;
    }
    g.h = height_axis;
    g.p0 = height_axis == 0 ? 1 : 0;
    g.p1 = height_axis == 2 ? 1 : 2;
    return SN_OK;
}

}  // namespace

extern "C" int sn_tower_centroids(const int64_t* stats, const int32_t* n_towers, int B, int max_towers, int height_axis,
                                  const double* voxel_size_host, const double* center_host, int apply_filter,
                                  double threshold, double tower_height, double rim_sq, double min_euc, uint8_t* keep,
                                  double* planar, double* agg, int32_t* n_agg, int32_t* status, sn_stream_t stream) {
    const char* who = "sn_tower_centroids";
    if (!stats || !n_towers || !keep || !agg || !n_agg || !status) return sn::fail(SN_ERR_INVALID_ARG, "%s: null pointer", who);
    if (B <= 0 || max_towers < 1) return sn::fail(SN_ERR_INVALID_ARG, "%s: B and max_towers must be positive", who);
    if (apply_filter && !center_host) return sn::fail(SN_ERR_INVALID_ARG, "%s: the filter needs center_host", who);
    Geom g;
    if (int e = geom_of(who, height_axis, voxel_size_host, center_host, g)) return e;
    if (!(min_euc > 0.0) || !std::isfinite(min_euc))
        return sn::fail(SN_ERR_INVALID_ARG, "%s: min_euc must be positive and finite", who);
    if (max_towers > kMaxRows || B > kMaxTiles)
        return sn::fail(SN_ERR_UNSUPPORTED, "%s: at most %d rows per tile and %d tiles (max_towers=%d, B=%d)", who, kMaxRows,
                        kMaxTiles, max_towers, B);
    if ((uintptr_t)stats % 8 || (uintptr_t)planar % 8 || (uintptr_t)agg % 8 || (uintptr_t)n_towers % 4 ||
        (uintptr_t)n_agg % 4 || (uintptr_t)status % 4)
        return sn::fail(SN_ERR_INVALID_ARG, "%s: stats / planar / agg must be aligned to 8 bytes, n_towers / n_agg / status to 4",
                        who);
    hipLaunchKernelGGL(tscore_centroids_kernel, dim3((unsigned)B), dim3(kThreads), 0, sn::as_stream(stream),
                       reinterpret_cast<const long long*>(stats), n_towers, max_towers, g, apply_filter, threshold,
                       tower_height, rim_sq, min_euc, keep, planar, agg, n_agg, status);
    return sn::check_launch("sn_tower_centroids");
}

extern "C" int sn_tower_match(const double* agg, const int32_t* n_agg, const int32_t* status_pred, int max_rows_pred,
                              const int64_t* gt_stats, const int32_t* gt_n_towers, int max_towers_gt, int B, int height_axis,
                              const double* voxel_size_host, double hit_dist, int32_t* match, double* dist, double* gt_planar,
                              int64_t* totals, double* dist_total, sn_stream_t stream) {
    const char* who = "sn_tower_match";
    if (!agg || !n_agg || !status_pred || !gt_stats || !gt_n_towers || !match || !dist)
        return sn::fail(SN_ERR_INVALID_ARG, "%s: null pointer", who);
    if ((totals == nullptr) != (dist_total == nullptr))
        return sn::fail(SN_ERR_INVALID_ARG, "%s: totals and dist_total go together", who);
    if (B <= 0 || max_rows_pred < 1 || max_towers_gt < 1)
        return sn::fail(SN_ERR_INVALID_ARG, "%s: B, max_rows_pred and max_towers_gt must be positive", who);
    Geom g;
    if (int e = geom_of(who, height_axis, voxel_size_host, nullptr, g)) return e;
    if (!(hit_dist > 0.0)) return sn::fail(SN_ERR_INVALID_ARG, "%s: hit_dist must be positive (+inf allowed)", who);
    if (max_rows_pred > kMaxRows || max_towers_gt > kMaxRows || B > kMaxTiles)
        return sn::fail(SN_ERR_UNSUPPORTED, "%s: at most %d rows per tile and %d tiles (max_rows_pred=%d, max_towers_gt=%d, B=%d)",
                        who, kMaxRows, kMaxTiles, max_rows_pred, max_towers_gt, B);
    if ((uintptr_t)agg % 8 || (uintptr_t)gt_stats % 8 || (uintptr_t)dist % 8 || (uintptr_t)gt_planar % 8 ||
        (uintptr_t)totals % 8 || (uintptr_t)dist_total % 8 || (uintptr_t)n_agg % 4 || (uintptr_t)status_pred % 4 ||
        (uintptr_t)gt_n_towers % 4 || (uintptr_t)match % 4)
        return sn::fail(SN_ERR_INVALID_ARG, "%s: agg / gt_stats / dist / gt_planar / totals / dist_total must be aligned to 8 "
                        "bytes, n_agg / status_pred / gt_n_towers / match to 4", who);
    hipStream_t s = sn::as_stream(stream);
    hipLaunchKernelGGL(tscore_match_kernel, dim3((unsigned)B), dim3(kThreads), 0, s, agg, n_agg, status_pred, max_rows_pred,
                       reinterpret_cast<const long long*>(gt_stats), gt_n_towers, max_towers_gt, g, hit_dist, match, dist,
                       gt_planar, reinterpret_cast<unsigned long long*>(totals));
    if (int e = sn::check_launch("sn_tower_match(match)")) return e;
    if (totals) {
        hipLaunchKernelGGL(tscore_dist_sum_kernel, dim3(1), dim3(kSumThreads), 0, s, match, dist, status_pred, gt_n_towers, B,
                           max_towers_gt, hit_dist, dist_total);
        if (int e = sn::check_launch("sn_tower_match(dist sum)")) return e;
    }
    return SN_OK;
}
