// K10 -- point DBSCAN: the towers of a labelled scan (sn_points_select, sn_dbscan_cell_grid, sn_dbscan_points).
// replaces: select_object -> extract_towers (utils/pcd_processing.py:508-522, 577-651: np.isin over the classes, open3d's
//           cluster_dbscan(eps=10, min_points=300) over the tower points of a whole scan and a pandas group-by, on the host)
//           in front of crop_tower_samples / crop_two_towers_samples (:765-817), hence of build_data_samples
//           (core/datasets/ts40k.py:86-92).
//
// Definition (normative, include/scenenet_hip.h): the selected points (label == keep[j] for some j; all without labels)
// keep scan order, their positions 0..m-1 are the indices below.  q is a neighbour of p iff
// (dx*dx + dy*dy) + dz*dz <= eps*eps in fp64 in exactly this form (this file is built with -ffp-contract=off), p itself
// included, the comparison literal (a NaN or infinite coordinate: nobody's neighbour, noise).  core: >= min_points
// neighbours; cluster: a connected component of the cores, ids ascending with the smallest core position; border: not core
// with a core neighbour, takes the smallest id among them; everything else -1.
//
// The selected positions are counting-sorted into the cell grid of cell_grid.h (cells from bounds' minimum), an
// accelerator only: the 9 runs of rows around a point's own cell hold every neighbour.
//   select:  count (members and the finite box per 1024 points) -> prefix (one workgroup) -> scatter (ballot + mbcnt: scan order)
//   1 cells    cell of every selected position, population per cell (integer atomics); status
//   2 prefix   cell_starts
//   3 scatter  scatter_row
//   4 core     neighbours counted over the 9 runs with an exit at min_points; parent[p] = p for a core, -1 otherwise
//   5 union    lock-free union-find over POSITIONS (union_find.h); each pair is taken once, by its larger position
//   6 flatten  parent[p] = root(p); a root's rank inside its 256 positions and the roots per 256 positions
//   7 rank     exclusive prefix of those counts (one workgroup): id = roots in front = rank by smallest core position;
//              n_clusters; stats zeroed
//   8 finish   cores take their root's id, borders the smallest root among their core neighbours; stats by integer atomics,
//              summed per wave first
// Home points of one wave mostly share their cell, so their candidate loads hit the same addresses (one transaction per
// wave).  Staging the runs through LDS and the dense-cell shortcut (cells of diagonal <= eps) are the next levers.
//
// Bound: launches 4, 5 and 8 by the latency of the candidate loads -- a distance test is 9 fp64 VALU operations behind a
// 32-byte row load that the lane waits for; measured 1.3e11 tests/s in the union, about 3 % of the part's fp64 vector
// rate.  The others by HBM / L2 latency.
#include "common.h"
#include "cell_grid.h"
#include "scan.h"
#include "union_find.h"
#include <cmath>

namespace {

constexpr int kThreads = 256;
constexpr int kSelGroups = 4;
constexpr int kSelChunk = kThreads * kSelGroups;   // scan points per workgroup of the select kernels
constexpr int kRankChunk = kThreads;               // positions per workgroup of launches 1, 3..6, 8
constexpr int kMaxKeep = 64;
constexpr int64_t kMaxN = (int64_t)1 << 33;
constexpr int kMaxClusters = 1 << 20;

// the neighbour test in exactly the documented form
__device__ __forceinline__ bool is_near(const Row& q, double x, double y, double z, double eps2) {
#pragma clang fp contract(off)
    const double dx = q.x - x, dy = q.y - y, dz = q.z - z;
    const double xx = dx * dx, yy = dy * dy, zz = dz * dz;
    return (xx + yy) + zz <= eps2;
}

// what the call clusters: min(n_sel, limit) positions; `told` is the count the caller states
struct Live {
    int m;
    bool over;
};
__device__ __forceinline__ Live live_rows(const int64_t* __restrict__ n_sel, int64_t fallback, int limit, int capacity) {
    const int64_t told = n_sel ? *n_sel : fallback;
    Live l;
    l.m = told <= 0 ? 0 : (told < limit ? (int)told : limit);
    l.over = told > capacity;
    return l;
}

// x, y, z of position i; a scan index outside the scan reads as NaN (noise) and never leaves the buffer
__device__ __forceinline__ void load_position(const double* __restrict__ pts, const int64_t* __restrict__ sel, int64_t n,
                                              int i, double& x, double& y, double& z) {
    const int64_t s = sel ? sel[i] : (int64_t)i;
    if ((uint64_t)s >= (uint64_t)n) {
        x = y = z = __longlong_as_double(0x7ff8000000000000ll);
        return;
    }
    x = pts[s * 3];
    y = pts[s * 3 + 1];
    z = pts[s * 3 + 2];
}

// ------------------------------------------------------------------------------------------------------------- select
__device__ __forceinline__ bool is_selected(const double* __restrict__ labels, const double* __restrict__ keep, int n_keep,
                                            int64_t i) {
    if (!labels) return true;
    const double l = labels[i];
    bool in = false;
    for (int j = 0; j < n_keep; ++j) in = in || l == keep[j];   // np.isin: a NaN equals nothing
    return in;
}

__device__ __forceinline__ bool is_finite64(double v) { return fabs(v) <= 1.7976931348623157e308; }   // (NaN compares false)

// workgroup c: counts[c] = selected points among its 1024, boxes[c] = min / max of their finite coordinates
__global__ __launch_bounds__(kThreads) void select_count_kernel(const double* __restrict__ pts,
                                                                const double* __restrict__ labels, int64_t n,
                                                                const double* __restrict__ keep, int n_keep,
                                                                int64_t* __restrict__ counts, double* __restrict__ boxes) {
    __shared__ int s_cnt[kThreads / 64];
    __shared__ double s_box[kThreads / 64][6];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t base = (int64_t)blockIdx.x * kSelChunk;
    const double inf = __longlong_as_double(0x7ff0000000000000ll);
    double lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
    int cnt = 0;
#pragma unroll
    for (int g = 0; g < kSelGroups; ++g) {
        const int64_t i = base + g * kThreads + threadIdx.x;
        if (i < n && is_selected(labels, keep, n_keep, i)) {
            ++cnt;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const double v = pts[i * 3 + a];
                if (is_finite64(v)) {
                    lo[a] = v < lo[a] ? v : lo[a];
                    hi[a] = v > hi[a] ? v : hi[a];
                }
            }
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        cnt += __shfl_xor(cnt, off, 64);
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double l = __shfl_xor(lo[a], off, 64), h = __shfl_xor(hi[a], off, 64);
            lo[a] = l < lo[a] ? l : lo[a];
            hi[a] = h > hi[a] ? h : hi[a];
        }
    }
    if (lane == 0) {
        s_cnt[wave] = cnt;
        for (int a = 0; a < 3; ++a) s_box[wave][a] = lo[a], s_box[wave][3 + a] = hi[a];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int total = 0;
        for (int w = 0; w < kThreads / 64; ++w) total += s_cnt[w];
        counts[blockIdx.x] = total;
    }
    if (threadIdx.x < 6) {
        const int a = threadIdx.x;
        double v = s_box[0][a];
        for (int w = 1; w < kThreads / 64; ++w) {
            const double t = s_box[w][a];
            v = a < 3 ? (t < v ? t : v) : (t > v ? t : v);
        }
        boxes[(int64_t)blockIdx.x * 6 + a] = v;
    }
}

// one workgroup: counts -> exclusive prefixes in place, n_sel; the boxes reduced into bbox (min and max of doubles: exact
// in any order)
__global__ __launch_bounds__(kScanThreads) void select_prefix_kernel(int64_t* __restrict__ counts,
                                                                     const double* __restrict__ boxes, int64_t nchunks,
                                                                     int64_t* __restrict__ n_sel, double* __restrict__ bbox) {
    __shared__ int64_t s_wave[kScanThreads / 64];
    __shared__ double s_box[kScanThreads / 64][6];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int64_t carry = 0;
    const double inf = __longlong_as_double(0x7ff0000000000000ll);
    double lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
    for (int64_t t0 = 0; t0 < nchunks; t0 += kScanThreads) {
        const int64_t c = t0 + threadIdx.x;
        int64_t v[1] = {c < nchunks ? counts[c] : 0};
        const int64_t total = sn::block_exclusive<kScanThreads, 1>(v, s_wave);
        if (c < nchunks) {
            counts[c] = carry + v[0];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const double l = boxes[c * 6 + a], h = boxes[c * 6 + 3 + a];
                lo[a] = l < lo[a] ? l : lo[a];
                hi[a] = h > hi[a] ? h : hi[a];
            }
        }
        carry += total;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double l = __shfl_xor(lo[a], off, 64), h = __shfl_xor(hi[a], off, 64);
            lo[a] = l < lo[a] ? l : lo[a];
            hi[a] = h > hi[a] ? h : hi[a];
        }
    if (lane == 0)
        for (int a = 0; a < 3; ++a) s_box[wave][a] = lo[a], s_box[wave][3 + a] = hi[a];
    __syncthreads();
    if (threadIdx.x < 6) {
        const int a = threadIdx.x;
        double v = s_box[0][a];
        for (int w = 1; w < kScanThreads / 64; ++w) {
            const double t = s_box[w][a];
            v = a < 3 ? (t < v ? t : v) : (t > v ? t : v);
        }
        bbox[a] = v;
    }
    if (threadIdx.x == 0) *n_sel = carry;
}

// sel[prefix + rank] = scan index: inside a workgroup the rank follows (group, wave, lane), which is scan order
__global__ __launch_bounds__(kThreads) void select_scatter_kernel(const double* __restrict__ labels, int64_t n,
                                                                  const double* __restrict__ keep, int n_keep,
                                                                  const int64_t* __restrict__ counts, int64_t capacity,
                                                                  int64_t* __restrict__ sel) {
    __shared__ int s_cnt[kSelGroups * (kThreads / 64)];
    const int wave = threadIdx.x >> 6;
    const int64_t base = (int64_t)blockIdx.x * kSelChunk;
    bool in[kSelGroups];
    int rank[kSelGroups];
#pragma unroll
    for (int g = 0; g < kSelGroups; ++g) {
        const int64_t i = base + g * kThreads + threadIdx.x;
        in[g] = i < n && is_selected(labels, keep, n_keep, i);
        const unsigned long long mask = __ballot(in[g]);
        rank[g] = sn::wave_rank(mask);
        if ((threadIdx.x & 63) == 0) s_cnt[g * (kThreads / 64) + wave] = __popcll(mask);
    }
    __syncthreads();
    const int64_t first = counts[blockIdx.x];
#pragma unroll
    for (int g = 0; g < kSelGroups; ++g) {
        int before = 0;
        for (int s = 0; s < g * (kThreads / 64) + wave; ++s) before += s_cnt[s];
        const int64_t o = first + before + rank[g];
        if (in[g] && (uint64_t)o < (uint64_t)capacity) sel[o] = base + g * kThreads + threadIdx.x;
    }
}

// ------------------------------------------------------------------------------------------------------------ cluster
// ---- 1: the cell of every position and the cells' populations (pop zeroed by a memset node in front); status
__global__ __launch_bounds__(kThreads) void dbscan_cells_kernel(const double* __restrict__ pts,
                                                                const int64_t* __restrict__ sel, int64_t n,
                                                                const int64_t* __restrict__ n_sel, int64_t fallback,
                                                                int limit, int capacity, CellGrid g,
                                                                int32_t* __restrict__ cell_of, int32_t* __restrict__ pop,
                                                                int32_t* __restrict__ status) {
    const Live l = live_rows(n_sel, fallback, limit, capacity);
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i == 0) *status = l.over ? 1 : 0;
    if (i >= l.m) return;
    double x, y, z;
    load_position(pts, sel, n, i, x, y, z);
    const int c = cell_of_point(g, x, y, z);
    cell_of[i] = c;
    atomicAdd(pop + c, 1);
}

// ---- 2: one workgroup: the cells' starts and cursors
__global__ __launch_bounds__(kScanThreads) void dbscan_prefix_kernel(int32_t* __restrict__ pop, int cells,
                                                                     int32_t* __restrict__ start) {
    __shared__ int64_t s_wave[kScanThreads / 64];
    cell_starts(pop, cells, start, s_wave);
}

// ---- 3: rows into cell order
__global__ __launch_bounds__(kThreads) void dbscan_scatter_kernel(const double* __restrict__ pts,
                                                                  const int64_t* __restrict__ sel, int64_t n,
                                                                  const int64_t* __restrict__ n_sel, int64_t fallback,
                                                                  int limit, int capacity,
                                                                  const int32_t* __restrict__ cell_of,
                                                                  int32_t* __restrict__ cursor, Row* __restrict__ rows) {
    const int m = live_rows(n_sel, fallback, limit, capacity).m;
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= m) return;
    Row r;
    load_position(pts, sel, n, i, r.x, r.y, r.z);
    r.pos = i;
    r.cell = cell_of[i];
    scatter_row(r, m, cursor, rows);
}

// ---- 4: core points.  parent[p] = p for a core, -1 for everything else
__global__ __launch_bounds__(kThreads) void dbscan_core_kernel(const int64_t* __restrict__ n_sel, int64_t fallback,
                                                               int limit, int capacity, CellGrid g, double eps2,
                                                               int min_points, const int32_t* __restrict__ start,
                                                               const Row* __restrict__ rows, int32_t* __restrict__ parent) {
    const int m = live_rows(n_sel, fallback, limit, capacity).m;
    const int r = blockIdx.x * kThreads + threadIdx.x;
    if (r >= m) return;
    const Row me = rows[r];
    int cnt = 0;
    for_candidates(g, start, rows, m, me.cell, [&](const Row& q) {
        cnt += is_near(q, me.x, me.y, me.z, eps2) ? 1 : 0;
        return cnt < min_points;
    });
    if ((unsigned)me.pos < (unsigned)m) parent[me.pos] = cnt >= min_points ? me.pos : -1;
}

// ---- union-find over parent[] (union_find.h): the indices are positions

// ---- 5: every core unites with its core neighbours of smaller position (the pair's other half is that one's business)
__global__ __launch_bounds__(kThreads) void dbscan_union_kernel(const int64_t* __restrict__ n_sel, int64_t fallback,
                                                                int limit, int capacity, CellGrid g, double eps2,
                                                                const int32_t* __restrict__ start,
                                                                const Row* __restrict__ rows, int32_t* __restrict__ parent) {
    const int m = live_rows(n_sel, fallback, limit, capacity).m;
    const int r = blockIdx.x * kThreads + threadIdx.x;
    if (r >= m) return;
    const Row me = rows[r];
    if ((unsigned)me.pos >= (unsigned)m || uf_load(parent + me.pos) < 0) return;   // cores never stop being cores
    int32_t root = me.pos;
    for_candidates(g, start, rows, m, me.cell, [&](const Row& q) {
        if (q.pos < me.pos && q.pos >= 0 && is_near(q, me.x, me.y, me.z, eps2)) {
            const int32_t pq = uf_load(parent + q.pos);
            if (pq >= 0 && pq != root) root = uf_unite(parent, root, q.pos);
        }
        return true;
    });
}

// ---- 6: parent[p] = root(p) for every core (no hooks happen in this launch: roots stay roots; parent[p] is written by p's
// own thread only, a reader sees the old ancestor or the root); a root's rank among the roots of its 256 positions
__global__ __launch_bounds__(kThreads) void dbscan_flatten_kernel(const int64_t* __restrict__ n_sel, int64_t fallback,
                                                                  int limit, int capacity, int32_t* __restrict__ parent,
                                                                  int32_t* __restrict__ root_rank,
                                                                  int32_t* __restrict__ chunk_roots) {
    __shared__ int s_cnt[kThreads / 64];
    const int m = live_rows(n_sel, fallback, limit, capacity).m;
    const int i = blockIdx.x * kThreads + threadIdx.x, wave = threadIdx.x >> 6;
    bool is_root = false;
    if (i < m && uf_load(parent + i) >= 0) {
        const int32_t r = uf_find_readonly(parent, i);
        if (r != i) uf_store(parent + i, r);
        is_root = r == i;
    }
    const unsigned long long mask = __ballot(is_root);
    if ((threadIdx.x & 63) == 0) s_cnt[wave] = __popcll(mask);
    __syncthreads();
    int before = 0, total = 0;
    for (int w = 0; w < kThreads / 64; ++w) {
        if (w < wave) before += s_cnt[w];
        total += s_cnt[w];
    }
    if (is_root) root_rank[i] = before + sn::wave_rank(mask);
    if (threadIdx.x == 0) chunk_roots[blockIdx.x] = total;
}

// ---- 7: one workgroup.  chunk_roots -> exclusive prefixes in place; n_clusters; stats zeroed
__global__ __launch_bounds__(kScanThreads) void dbscan_rank_kernel(int32_t* __restrict__ chunk_roots, int nchunks,
                                                                   int max_clusters, int32_t* __restrict__ n_clusters,
                                                                   long long* __restrict__ stats) {
    __shared__ int32_t s_wave[kScanThreads / 64];
    // (int32 throughout, as the slots are: the roots are positions, fewer than 2^31)
    const int32_t roots = sn::scan_row<kScanThreads, 1>(chunk_roots, nchunks, s_wave);
    for (int i = threadIdx.x; i < max_clusters * SN_DBSCAN_NSTAT; i += kScanThreads) stats[i] = 0;
    if (threadIdx.x == 0) *n_clusters = roots;
}

// ---- 8: labels and statistics
__global__ __launch_bounds__(kThreads) void dbscan_finish_kernel(const int64_t* __restrict__ sel,
                                                                 const int64_t* __restrict__ n_sel, int64_t fallback,
                                                                 int limit, int capacity, CellGrid g, double eps2,
                                                                 const int32_t* __restrict__ start,
                                                                 const Row* __restrict__ rows,
                                                                 const int32_t* __restrict__ parent,
                                                                 const int32_t* __restrict__ root_rank,
                                                                 const int32_t* __restrict__ chunk_roots, int max_clusters,
                                                                 int32_t* __restrict__ cluster, long long* __restrict__ stats) {
    const int m = live_rows(n_sel, fallback, limit, capacity).m;
    const int r = blockIdx.x * kThreads + threadIdx.x, lane = threadIdx.x & 63;
    int32_t id = -1;
    bool core = false;
    int pos = -1;
    if (r < m) {
        const Row me = rows[r];
        if ((unsigned)me.pos < (unsigned)m) {
            pos = me.pos;
            int32_t root = parent[pos];
            core = root >= 0;
            if (!core) {
                // border: the smallest root among the core neighbours = the smallest cluster id
                int32_t best = 0x7fffffff;
                for_candidates(g, start, rows, m, me.cell, [&](const Row& q) {
                    if ((unsigned)q.pos < (unsigned)m && is_near(q, me.x, me.y, me.z, eps2)) {
                        const int32_t pq = parent[q.pos];
                        if (pq >= 0 && pq < best) best = pq;
                    }
                    return true;
                });
                if (best != 0x7fffffff) root = best;
            }
            if (root >= 0) id = chunk_roots[root / kRankChunk] + root_rank[root];
            cluster[pos] = id;
            if (core && root == pos && id < max_clusters) stats[(size_t)id * SN_DBSCAN_NSTAT + 2] = sel ? sel[pos] : (int64_t)pos;
        }
    }
    // statistics: the lanes of one cluster are counted in the wave, one lane adds
    const bool has = id >= 0 && id < max_clusters;
    unsigned long long todo = __ballot(has);
    unsigned long long* rowsum = reinterpret_cast<unsigned long long*>(stats);
    while (todo) {
        const int leader = __ffsll(todo) - 1;
        const int32_t lid = __shfl(id, leader, 64);
        const bool mine = has && id == lid;
        const unsigned long long mm = __ballot(mine), mc = __ballot(mine && core);
        todo &= ~mm;
        if (lane == leader) {
            atomicAdd(rowsum + (size_t)lid * SN_DBSCAN_NSTAT + 0, (unsigned long long)__popcll(mm));
            if (mc) atomicAdd(rowsum + (size_t)lid * SN_DBSCAN_NSTAT + 1, (unsigned long long)__popcll(mc));
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------ host
int64_t select_chunks(int64_t n) { return (n + kSelChunk - 1) / kSelChunk; }

// dims of the grid with cells of side cell_side(k, eps); false if it has more than max_cells cells
bool dims_at(const double* extent, double eps, double k, int64_t max_cells, int* dim, double* side_out) {
    const double side = cell_side(k, eps);
    int64_t cells = 1;
    for (int a = 0; a < 3; ++a) {
        const double d = std::floor(extent[a] / side) + 1.0;
        if (!(d <= (double)max_cells)) return false;
        cells *= (int64_t)d;
        if (cells > max_cells) return false;
        dim[a] = (int)d;
    }
    *side_out = side;
    return true;
}

int cell_grid(const char* who, const double* b, double eps, int64_t max_cells, CellGrid& g, double* side_out) {
    if (!b) return sn::fail(SN_ERR_INVALID_ARG, "%s: bounds_host is null", who);
    if (!(eps > 0.0) || !std::isfinite(eps)) return sn::fail(SN_ERR_INVALID_ARG, "%s: eps must be positive and finite", who);
    if (max_cells < 1) return sn::fail(SN_ERR_INVALID_ARG, "%s: max_cells must be at least 1", who);
    double extent[3];
    for (int a = 0; a < 3; ++a) {
        extent[a] = b[3 + a] - b[a];
        if (!std::isfinite(b[a]) || !std::isfinite(b[3 + a]) || !(extent[a] >= 0.0) || !std::isfinite(extent[a]))
            return sn::fail(SN_ERR_INVALID_ARG, "%s: bounds must be finite with max >= min on every axis", who);
    }
    if (eps < kEpsMin || eps > kEpsMax)
        return sn::fail(SN_ERR_UNSUPPORTED, "%s: eps beyond what is served (1e-150 .. 1e150)", who);
    if (max_cells > kMaxCells)
        return sn::fail(SN_ERR_UNSUPPORTED, "%s: max_cells beyond what is served (at most %lld)", who, (long long)kMaxCells);
    double side = 0.0;
    double k_bad = 0.0, k_ok = 1.0;   // the smallest k that fits lies in (k_bad, k_ok]; the cell count never grows with k
    while (!dims_at(extent, eps, k_ok, max_cells, g.dim, &side)) {
        k_bad = k_ok;
        k_ok *= 2.0;   // (ends: an infinite side holds everything in one cell)
    }
    while (k_ok - k_bad > 1.0) {
        const double mid = std::floor(k_bad + (k_ok - k_bad) / 2.0);
        if (!(mid > k_bad && mid < k_ok)) break;   // beyond 2^53 the doubles themselves are the integers
        if (dims_at(extent, eps, mid, max_cells, g.dim, &side)) k_ok = mid;
        else k_bad = mid;
    }
    dims_at(extent, eps, k_ok, max_cells, g.dim, &side);
    for (int a = 0; a < 3; ++a) g.lo[a] = b[a];
    g.inv = 1.0 / side;
    g.cells = g.dim[0] * g.dim[1] * g.dim[2];
    if (side_out) *side_out = side;
    return SN_OK;
}

struct Layout {
    size_t cell_of, parent, root_rank, chunk_roots, start, pop, rows, bytes;
    int nchunks;
};
bool layout_of(int64_t capacity, int64_t cells, Layout& L) {
    if (capacity < 1 || capacity >= ((int64_t)1 << 31) || cells < 1 || cells > kMaxCells) return false;
    const size_t C = (size_t)capacity;
    auto pad = [](size_t v) { return (v + 15) / 16 * 16; };
    L.nchunks = (int)((capacity + kRankChunk - 1) / kRankChunk);
    size_t at = 0;
    L.rows = at, at += C * sizeof(Row);
    L.cell_of = at, at += pad(C * 4);
    L.parent = at, at += pad(C * 4);
    L.root_rank = at, at += pad(C * 4);
    L.chunk_roots = at, at += pad((size_t)L.nchunks * 4);
    L.start = at, at += pad(((size_t)cells + 1) * 4);
    L.pop = at, at += pad((size_t)cells * 4);
    L.bytes = at;
    return true;
}

int run(const double* pts, int64_t n, const int64_t* sel, const int64_t* n_sel, int64_t capacity, const double* bounds_host,
        double eps, int min_points, int64_t max_cells, int max_clusters, void* ws, size_t ws_bytes, int32_t* cluster,
        int32_t* n_clusters, int64_t* stats, int32_t* status, int first, int last, sn_stream_t stream) {
    const char* who = "sn_dbscan_points";
    if (!pts || !ws || !cluster || !n_clusters || !status) return sn::fail(SN_ERR_INVALID_ARG, "%s: null pointer", who);
    if (sel && !n_sel) return sn::fail(SN_ERR_INVALID_ARG, "%s: n_sel is null though sel is given", who);
    if (n <= 0) return sn::fail(SN_ERR_INVALID_ARG, "%s: n must be positive (got %lld)", who, (long long)n);
    if (capacity <= 0) return sn::fail(SN_ERR_INVALID_ARG, "%s: capacity must be positive (got %lld)", who, (long long)capacity);
    if (min_points < 1) return sn::fail(SN_ERR_INVALID_ARG, "%s: min_points must be at least 1", who);
    if (max_clusters < 0 || (max_clusters > 0 && !stats))
        return sn::fail(SN_ERR_INVALID_ARG, "%s: max_clusters must not be negative, and stats is needed unless it is 0", who);
    CellGrid g;
    if (int e = cell_grid(who, bounds_host, eps, max_cells, g, nullptr)) return e;
    if (capacity >= ((int64_t)1 << 31) || n > kMaxN || max_clusters > kMaxClusters)
        return sn::fail(SN_ERR_UNSUPPORTED, "%s: capacity < 2^31, n <= 2^33 and max_clusters <= 2^20 are served", who);
    if ((uintptr_t)pts % 8 || (uintptr_t)sel % 8 || (uintptr_t)n_sel % 8 || (uintptr_t)ws % 16 || (uintptr_t)cluster % 4 ||
        (uintptr_t)n_clusters % 4 || (uintptr_t)stats % 8 || (uintptr_t)status % 4)
        return sn::fail(SN_ERR_INVALID_ARG, "%s: pts / sel / n_sel / stats must be 8-byte aligned, ws 16-byte, cluster / "
                        "n_clusters / status 4-byte", who);
    Layout L;
    layout_of(capacity, g.cells, L);
    if (ws_bytes < L.bytes)
        return sn::fail(SN_ERR_INVALID_ARG, "%s: ws holds %zu bytes, %zu needed (sn_dbscan_ws_bytes)", who, ws_bytes, L.bytes);

    hipStream_t s = sn::as_stream(stream);
    char* w = static_cast<char*>(ws);
    Row* rows = reinterpret_cast<Row*>(w + L.rows);
    int32_t* cell_of = reinterpret_cast<int32_t*>(w + L.cell_of);
    int32_t* parent = reinterpret_cast<int32_t*>(w + L.parent);
    int32_t* root_rank = reinterpret_cast<int32_t*>(w + L.root_rank);
    int32_t* chunk_roots = reinterpret_cast<int32_t*>(w + L.chunk_roots);
    int32_t* start = reinterpret_cast<int32_t*>(w + L.start);
    int32_t* pop = reinterpret_cast<int32_t*>(w + L.pop);
    // without sel the positions are the scan's own rows: never more than n of them
    const int limit = (int)(!sel && n < capacity ? n : capacity);
    const int64_t fallback = n;
    const double eps2 = eps * eps;
    const dim3 grid((unsigned)((limit + kThreads - 1) / kThreads)), block(kThreads);
    long long* st64 = reinterpret_cast<long long*>(stats);

    if (first <= 1 && last >= 1) {
        if (hipMemsetAsync(pop, 0, (size_t)g.cells * 4, s) != hipSuccess)
            return sn::fail(SN_ERR_LAUNCH, "%s: hipMemsetAsync failed", who);
        hipLaunchKernelGGL(dbscan_cells_kernel, grid, block, 0, s, pts, sel, n, n_sel, fallback, limit, (int)capacity, g,
                           cell_of, pop, status);
        if (int e = sn::check_launch("sn_dbscan_points(cells)")) return e;
    }
    if (first <= 2 && last >= 2) {
        hipLaunchKernelGGL(dbscan_prefix_kernel, dim3(1), dim3(kScanThreads), 0, s, pop, g.cells, start);
        if (int e = sn::check_launch("sn_dbscan_points(prefix)")) return e;
    }
    if (first <= 3 && last >= 3) {
        hipLaunchKernelGGL(dbscan_scatter_kernel, grid, block, 0, s, pts, sel, n, n_sel, fallback, limit, (int)capacity,
                           cell_of, pop, rows);
        if (int e = sn::check_launch("sn_dbscan_points(scatter)")) return e;
    }
    if (first <= 4 && last >= 4) {
        hipLaunchKernelGGL(dbscan_core_kernel, grid, block, 0, s, n_sel, fallback, limit, (int)capacity, g, eps2, min_points,
                           start, rows, parent);
        if (int e = sn::check_launch("sn_dbscan_points(core)")) return e;
    }
    if (first <= 5 && last >= 5) {
        hipLaunchKernelGGL(dbscan_union_kernel, grid, block, 0, s, n_sel, fallback, limit, (int)capacity, g, eps2, start, rows,
                           parent);
        if (int e = sn::check_launch("sn_dbscan_points(union)")) return e;
    }
    if (first <= 6 && last >= 6) {
        hipLaunchKernelGGL(dbscan_flatten_kernel, dim3((unsigned)L.nchunks), block, 0, s, n_sel, fallback, limit,
                           (int)capacity, parent, root_rank, chunk_roots);
        if (int e = sn::check_launch("sn_dbscan_points(flatten)")) return e;
    }
    if (first <= 7 && last >= 7) {
        hipLaunchKernelGGL(dbscan_rank_kernel, dim3(1), dim3(kScanThreads), 0, s, chunk_roots, L.nchunks, max_clusters,
                           n_clusters, st64);
        if (int e = sn::check_launch("sn_dbscan_points(rank)")) return e;
    }
    if (first <= 8 && last >= 8) {
        hipLaunchKernelGGL(dbscan_finish_kernel, grid, block, 0, s, sel, n_sel, fallback, limit, (int)capacity, g, eps2, start,
                           rows, parent, root_rank, chunk_roots, max_clusters, cluster, st64);
        if (int e = sn::check_launch("sn_dbscan_points(finish)")) return e;
    }
    return SN_OK;
}

}  // namespace

extern "C" int sn_points_select_chunk_points(void) { return kSelChunk; }
extern "C" int sn_dbscan_chunk_points(void) { return kRankChunk; }

extern "C" size_t sn_points_select_ws_bytes(int64_t n) {
    if (n <= 0 || n > kMaxN) return 0;
    return (size_t)select_chunks(n) * 7 * 8;   // a count and a box of six per workgroup
}

extern "C" int sn_points_select(const double* pts, const double* labels, int64_t n, const double* keep, int n_keep,
                                int64_t capacity, void* ws, size_t ws_bytes, int64_t* sel, int64_t* n_sel, double* bbox,
                                sn_stream_t stream) {
    const char* who = "sn_points_select";
    if (!pts || !ws || !n_sel || !bbox) return sn::fail(SN_ERR_INVALID_ARG, "%s: null pointer (pts, ws, n_sel, bbox)", who);
    if (labels && !keep) return sn::fail(SN_ERR_INVALID_ARG, "%s: keep is null though labels are given", who);
    if (n <= 0) return sn::fail(SN_ERR_INVALID_ARG, "%s: n must be positive (got %lld)", who, (long long)n);
    if (labels && n_keep < 0) return sn::fail(SN_ERR_INVALID_ARG, "%s: n_keep must not be negative", who);
    if (capacity < 0 || (capacity > 0 && !sel))
        return sn::fail(SN_ERR_INVALID_ARG, "%s: capacity must not be negative, and sel is needed unless it is 0", who);
    if (n > kMaxN || (labels && n_keep > kMaxKeep))
        return sn::fail(SN_ERR_UNSUPPORTED, "%s: n <= 2^33 and n_keep <= %d are served", who, kMaxKeep);
    if ((uintptr_t)pts % 8 || (uintptr_t)labels % 8 || (uintptr_t)keep % 8 || (uintptr_t)ws % 8 || (uintptr_t)sel % 8 ||
        (uintptr_t)n_sel % 8 || (uintptr_t)bbox % 8)
        return sn::fail(SN_ERR_INVALID_ARG, "%s: every pointer must be 8-byte aligned", who);
    if (ws_bytes < sn_points_select_ws_bytes(n))
        return sn::fail(SN_ERR_INVALID_ARG, "%s: ws holds %zu bytes, %zu needed (sn_points_select_ws_bytes)", who, ws_bytes,
                        sn_points_select_ws_bytes(n));
    hipStream_t s = sn::as_stream(stream);
    const int64_t nchunks = select_chunks(n);
    int64_t* counts = static_cast<int64_t*>(ws);
    double* boxes = reinterpret_cast<double*>(counts + nchunks);
    hipLaunchKernelGGL(select_count_kernel, dim3((unsigned)nchunks), dim3(kThreads), 0, s, pts, labels, n, keep, n_keep,
                       counts, boxes);
    hipLaunchKernelGGL(select_prefix_kernel, dim3(1), dim3(kScanThreads), 0, s, counts, boxes, nchunks, n_sel, bbox);
    if (capacity > 0)
        hipLaunchKernelGGL(select_scatter_kernel, dim3((unsigned)nchunks), dim3(kThreads), 0, s, labels, n, keep, n_keep,
                           counts, capacity, sel);
    return sn::check_launch(who);
}

extern "C" int sn_dbscan_cell_grid(const double* bounds_host, double eps, int64_t max_cells, int32_t* dims_out,
                                   double* side_out) {
    CellGrid g;
    if (int e = cell_grid("sn_dbscan_cell_grid", bounds_host, eps, max_cells, g, side_out)) return e;
    if (dims_out)
        for (int a = 0; a < 3; ++a) dims_out[a] = g.dim[a];
    return SN_OK;
}

extern "C" size_t sn_dbscan_ws_bytes(int64_t capacity, int64_t cells) {
    Layout L;
    return layout_of(capacity, cells, L) ? L.bytes : 0;
}

extern "C" int sn_dbscan_points(const double* pts, int64_t n, const int64_t* sel, const int64_t* n_sel, int64_t capacity,
                                const double* bounds_host, double eps, int min_points, int64_t max_cells, int max_clusters,
                                void* ws, size_t ws_bytes, int32_t* cluster, int32_t* n_clusters, int64_t* stats,
                                int32_t* status, sn_stream_t stream) {
    return run(pts, n, sel, n_sel, capacity, bounds_host, eps, min_points, max_cells, max_clusters, ws, ws_bytes, cluster,
               n_clusters, stats, status, 1, SN_DBSCAN_LAUNCHES, stream);
}

extern "C" int sn_dbscan_points_launches(const double* pts, int64_t n, const int64_t* sel, const int64_t* n_sel,
                                         int64_t capacity, const double* bounds_host, double eps, int min_points,
                                         int64_t max_cells, int max_clusters, void* ws, size_t ws_bytes, int32_t* cluster,
                                         int32_t* n_clusters, int64_t* stats, int32_t* status, int first, int last,
                                         sn_stream_t stream) {
    if (first < 1 || last > SN_DBSCAN_LAUNCHES || first > last)
        return sn::fail(SN_ERR_INVALID_ARG, "sn_dbscan_points_launches: 1 <= first <= last <= %d", SN_DBSCAN_LAUNCHES);
    return run(pts, n, sel, n_sel, capacity, bounds_host, eps, min_points, max_cells, max_clusters, ws, ws_bytes, cluster,
               n_clusters, stats, status, first, last, stream);
}
