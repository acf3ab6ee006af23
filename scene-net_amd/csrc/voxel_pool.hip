// K24 -- voxel pooling: up to eight planes per voxel of a CSR batch, each the mean, the minimum or the maximum of a
// coordinate or of a per-point value column over the rows K1's rule bins into the voxel, and the rows' count.
// replaces: Vox.centroid_hist_on_voxel / Vox.centroid_reg_on_voxel, which core/datasets/torch_transforms.py:161-162 calls
//           and the reference's tree does not contain (build-defined: the mean position of a voxel's points); and the
//           torch formulation index_add_ / scatter_reduce over flat indices built by searchsorted.
//
// Definition (normative, include/scenenet_hip.h).  A row is binned by sn::Binner::flat (binning.h: the text voxel.hip,
// thin.hip and voxel_classes.hip bin with).  MEAN is a fixed-point mean: q = rint(clamp(fl(fl(p - lo) * inv), 0, 2^32)),
// S = the integer sum of the q, decoded as fl(lo + fl(fl((double)S / (double)n) * step)).  MIN / MAX reduce the
// order-preserving key of common.h (enc_f64) by integer atomic min / max.  Integer sums, minima and maxima: the bits do not
// depend on scheduling or on the order of the rows.
//
// Shape: voxel_classes.hip's -- one WAVE per workgroup, kWaveChunk = 1024 consecutive rows of the packed batch, the tiles
// that reach into the chunk walked (sn::for_tiles, packed_rows.h) one edge table in LDS at a time; next to the table the
// tile's quantisers (lo, inv per plane), formed by the first P lanes.
//   clear     accumulators <- what each reduction starts from (0 for a count, a sum and a maximum, all ones for a
//             minimum), unbinned, nan_rows <- 0 (one kernel, no memset node: see voxel_classes.hip's zero_kernel)
//   rows      per row that takes part: one integer atomic add for the count and one 64-bit integer atomic per plane; a
//             min / max atomic is sent only where a plain load of the cell shows it can still change the cell (the cell only
//             moves one way: a stale look costs a needless atomic, never a result)
//   decode    sums and keys -> planes, in place; `fill` where the count is 0
// The accumulators live in the outputs themselves: `out`'s cells hold the sums and keys, `counts` the counts, and decode
// rewrites `out` in place, so the call needs no workspace.  A row's P + 1 atomics go to P + 1 lines that lie 8 V bytes apart.
// [measured] the other home -- a workspace of P + 1 consecutive words per voxel, so that a row's atomics share one or two
// lines -- was built and timed on 32 tiles of 10^5 points at 64^3: 1.07x (P = 1), 1.13x (P = 3) and 1.11x (P = 8) the time
// of this one (the atomics run at the memory side either way; it clears and decodes (P + 1) * 8 more bytes per voxel).
// It was taken out again.  Not measured: grids with few rows per occupied voxel, where the lines might matter more.
//
// Bound: rows reads 24 B + 8 B per value column per row; the outputs, P * 8 + 4 B per voxel, are written three times over
// (clear, the atomics' lines, decode).
#include <cstring>
#include "common.h"
#include "binning.h"
#include "packed_rows.h"
#include "scan.h"

namespace {

using sn::kWaveLanes;
using sn::kWaveGroups;
using sn::kWaveChunk;
constexpr int kMaxB = 1 << 16;
constexpr int kMaxP = SN_POOL_MAX_PLANES, kMaxC = SN_POOL_MAX_COLUMNS;
constexpr int64_t kMaxTotal = ((int64_t)1 << 31) - 1;
constexpr double kTwo32 = 4294967296.0;
constexpr unsigned long long kAllOnes = ~0ull;

// what the three kernels need of the planes: by value, so that a captured call keeps what it was given
struct Plan {
    int P, C;
    unsigned used;          // bit c: some plane reads value column c
    int src[kMaxP];         // 0, 1, 2: x, y, z; 3 + c: value column c
    int op[kMaxP];
    double lo[kMaxP];       // a value source's range (a coordinate source takes the tile's box from desc)
    double hi[kMaxP];
    unsigned long long fill;
};

__device__ __forceinline__ unsigned long long start_of(int op) { return op == SN_POOL_MIN ? kAllOnes : 0ull; }

// plane p's lo and span for tile descriptor d
__device__ __forceinline__ void range_of(const Plan& plan, int p, const double* __restrict__ d, double& lo, double& span) {
    const int s = plan.src[p];
    const double hi = s < 3 ? d[3 + s] : plan.hi[p];
    lo = s < 3 ? d[s] : plan.lo[p];
    span = hi - lo;
}

// ---------------------------------------------------------------- clear
// out[b][p][.] <- the start of plane p, counts <- 0: blockIdx.y walks the (tile, slot) pairs, slot 0 the counts
__global__ __launch_bounds__(256) void pool_clear_kernel(Plan plan, int B, int64_t V, unsigned long long* __restrict__ acc,
                                                         int32_t* __restrict__ counts, unsigned long long* __restrict__ unbinned,
                                                         unsigned long long* __restrict__ nan_rows) {
    const int64_t stride = (int64_t)gridDim.x * 256, first = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int P = plan.P;
    if (blockIdx.y == 0)
        for (int64_t i = first; i < B; i += stride) {
            unbinned[i] = 0ull;
            nan_rows[i] = 0ull;
        }
    for (int bp = blockIdx.y; bp < B * (P + 1); bp += gridDim.y) {
        const int b = bp / (P + 1), slot = bp % (P + 1);
        if (slot == 0) {
            int32_t* mine = counts + (size_t)b * (size_t)V;
            for (int64_t i = first; i < V; i += stride) mine[i] = 0;
        } else {
            unsigned long long* mine = acc + ((size_t)b * P + (slot - 1)) * (size_t)V;
            const unsigned long long v = start_of(plan.op[slot - 1]);
            for (int64_t i = first; i < V; i += stride) mine[i] = v;
        }
    }
}

// ---------------------------------------------------------------- rows
template <bool kLook>
__global__ __launch_bounds__(kWaveLanes) void pool_rows_kernel(Plan plan, const double* __restrict__ pts,
                                                               const double* __restrict__ values,
                                                               const int64_t* __restrict__ offsets, int64_t total, int B,
                                                               const double* __restrict__ desc, int nx, int ny, int nz,
                                                               unsigned long long* __restrict__ acc, int32_t* __restrict__ counts,
                                                               unsigned long long* __restrict__ unbinned,
                                                               unsigned long long* __restrict__ nan_rows) {
    extern __shared__ double edges[];
    __shared__ double s_lo[kMaxP], s_inv[kMaxP];
    const int lane = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * kWaveChunk;
    const int ne = nx + ny + nz + 3;
    const int64_t V = (int64_t)nx * ny * nz;
    const int P = plan.P, C = plan.C;
    sn::for_tiles(offsets, B, base, kWaveChunk, total, [&](int b, int64_t, int64_t, int64_t from, int64_t to) {
        const double* d = desc + (size_t)b * (size_t)(6 + ne);
        __syncthreads();   // the previous tile's table and quantisers have been read
        if (lane < P) {
            double qlo, span;
            range_of(plan, lane, d, qlo, span);
            const double inv = kTwo32 / span;
            s_lo[lane] = qlo;
            s_inv[lane] = (span > 0.0 && inv <= DBL_MAX) ? inv : 0.0;   // (a NaN span fails the first test)
        }
        sn::load_edges(edges, d, ne, kWaveLanes);   // (ends in a barrier)
        sn::Binner bin;
        bin.init(edges, d, nx, ny, nz);
        int nunb = 0, nnan = 0;
#pragma unroll 2
        for (int g = 0; g < kWaveGroups; ++g) {
            const int64_t i = base + g * kWaveLanes + lane;
            const bool mine = i >= from && i < to;
            bool unb = false, isnan = false;
            if (mine) {
                const double* p = pts + i * 3;
                const double x = p[0], y = p[1], z = p[2];
                const int f = bin.flat(x, y, z);
                unb = f < 0;
                const double* row = values + i * C;   // (read only where a plane reads a column: `values` may be null)
                if (!unb) {
                    for (int c = 0; c < C; ++c)
                        if (plan.used >> c & 1u) {
                            const double v = row[c];
                            isnan |= v != v;
                        }
                }
                if (!unb && !isnan) {
                    __hip_atomic_fetch_add(counts + (size_t)b * (size_t)V + (size_t)f, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    unsigned long long* cell = acc + (size_t)b * (size_t)P * (size_t)V + (size_t)f;
                    for (int q = 0; q < P; ++q, cell += V) {
                        const int s = plan.src[q], op = plan.op[q];
                        const double v = s == 0 ? x : s == 1 ? y : s == 2 ? z : row[s - 3];
                        if (op == SN_POOL_MEAN) {
                            double t = (v - s_lo[q]) * s_inv[q];
                            t = t > 0.0 ? t : 0.0;            // (a NaN product -- an infinite difference times inv = 0 -- is 0)
                            t = t < kTwo32 ? t : kTwo32;
                            __hip_atomic_fetch_add(cell, (unsigned long long)(long long)rint(t), __ATOMIC_RELAXED,
                                                   __HIP_MEMORY_SCOPE_AGENT);
                        } else {
                            const unsigned long long key = sn::enc_f64(v);
                            if (op == SN_POOL_MAX) {
                                if (!kLook || __hip_atomic_load(cell, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < key)
                                    __hip_atomic_fetch_max(cell, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                            } else {
                                if (!kLook || __hip_atomic_load(cell, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > key)
                                    __hip_atomic_fetch_min(cell, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                            }
                        }
                    }
                }
            }
            nunb += __popcll(__ballot(unb));
            nnan += __popcll(__ballot(isnan));
        }
        if (lane == 0) {
            if (nunb) __hip_atomic_fetch_add(unbinned + b, (unsigned long long)nunb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (nnan) __hip_atomic_fetch_add(nan_rows + b, (unsigned long long)nnan, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    });
}

// ---------------------------------------------------------------- decode
__device__ __forceinline__ unsigned long long decoded(int op, unsigned long long a, int64_t n, double lo, double step) {
    if (op == SN_POOL_MEAN) {
        const double m = (double)(long long)a / (double)n;
        return (unsigned long long)__double_as_longlong(lo + m * step);
    }
    return (unsigned long long)__double_as_longlong(sn::dec_f64(a));
}

// in place; blockIdx.y walks the (tile, plane) pairs
__global__ __launch_bounds__(256) void pool_decode_kernel(Plan plan, int B, int64_t V, const double* __restrict__ desc,
                                                          int desc_len, unsigned long long* __restrict__ out,
                                                          const int32_t* __restrict__ counts) {
    const int64_t stride = (int64_t)gridDim.x * 256, first = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int P = plan.P;
    for (int bp = blockIdx.y; bp < B * P; bp += gridDim.y) {
        const int b = bp / P, p = bp % P;
        double lo, span;
        range_of(plan, p, desc + (size_t)b * (size_t)desc_len, lo, span);
        const double step = span / kTwo32;
        const int op = plan.op[p];
        unsigned long long* mine = out + (size_t)bp * (size_t)V;
        const int32_t* cnt = counts + (size_t)b * (size_t)V;
        for (int64_t v = first; v < V; v += stride) {
            const int64_t n = cnt[v];
            mine[v] = n == 0 ? plan.fill : decoded(op, mine[v], n, lo, step);
        }
    }
}

}  // namespace

extern "C" int sn_voxel_pool_chunk_points(void) { return kWaveChunk; }

// the call accumulates in `out` and `counts`: no workspace for any shape
extern "C" int64_t sn_voxel_pool_ws_bytes(int, int, int, int, int) { return 0; }

extern "C" int sn_voxel_pool(const double* pts, const double* values, int C, const int64_t* offsets, int64_t total, int B,
                             const double* desc, int nx, int ny, int nz, const int32_t* plane_source_host,
                             const int32_t* plane_op_host, int P, const double* value_range_host, double fill, int flags,
                             void* ws, double* out, int32_t* counts, int64_t* unbinned, int64_t* nan_rows,
                             sn_stream_t stream) {
    const char* what = "sn_voxel_pool";
    if (!pts) return sn::fail(SN_ERR_INVALID_ARG, "%s: pts is null", what);
    if (!offsets) return sn::fail(SN_ERR_INVALID_ARG, "%s: offsets is null", what);
    if (!desc) return sn::fail(SN_ERR_INVALID_ARG, "%s: desc is null", what);
    if (!out) return sn::fail(SN_ERR_INVALID_ARG, "%s: out is null", what);
    if (!counts) return sn::fail(SN_ERR_INVALID_ARG, "%s: counts is null", what);
    if (!unbinned) return sn::fail(SN_ERR_INVALID_ARG, "%s: unbinned is null", what);
    if (!nan_rows) return sn::fail(SN_ERR_INVALID_ARG, "%s: nan_rows is null", what);
    if (!plane_source_host || !plane_op_host) return sn::fail(SN_ERR_INVALID_ARG, "%s: the plane lists are null", what);
    if (C < 0 || C > kMaxC) return sn::fail(SN_ERR_INVALID_ARG, "%s: C must be 0 .. %d (got %d)", what, kMaxC, C);
    if (P < 1 || P > kMaxP) return sn::fail(SN_ERR_INVALID_ARG, "%s: P must be 1 .. %d (got %d)", what, kMaxP, P);
    if (flags & ~SN_VOXEL_POOL_NO_LOOK) return sn::fail(SN_ERR_INVALID_ARG, "%s: unknown flags %d", what, flags);
    Plan plan;
    memset(&plan, 0, sizeof(plan));
    plan.P = P;
    plan.C = C;
    memcpy(&plan.fill, &fill, sizeof(fill));
    for (int p = 0; p < P; ++p) {
        const int s = plane_source_host[p], op = plane_op_host[p];
        if (s < 0 || s >= 3 + C)
            return sn::fail(SN_ERR_INVALID_ARG, "%s: plane %d reads source %d, beyond 3 + C = %d", what, p, s, 3 + C);
        if (op != SN_POOL_MEAN && op != SN_POOL_MIN && op != SN_POOL_MAX)
            return sn::fail(SN_ERR_INVALID_ARG, "%s: plane %d has the unknown op %d", what, p, op);
        plan.src[p] = s;
        plan.op[p] = op;
        if (s < 3) continue;
        plan.used |= 1u << (s - 3);
        if (!values) return sn::fail(SN_ERR_INVALID_ARG, "%s: values is null and plane %d reads column %d", what, p, s - 3);
        if (op != SN_POOL_MEAN) continue;
        if (!value_range_host)
            return sn::fail(SN_ERR_INVALID_ARG, "%s: value_range is null and plane %d takes the mean of column %d", what, p, s - 3);
        const double lo = value_range_host[2 * (s - 3)], hi = value_range_host[2 * (s - 3) + 1];
        if (!(lo >= -DBL_MAX && hi <= DBL_MAX && hi > lo))
            return sn::fail(SN_ERR_INVALID_ARG, "%s: the value range of column %d must be finite with hi > lo (got %g, %g)", what,
                            s - 3, lo, hi);
        plan.lo[p] = lo;
        plan.hi[p] = hi;
    }
    if (total <= 0) return sn::fail(SN_ERR_INVALID_ARG, "%s: total must be positive (got %lld)", what, (long long)total);
    if (B <= 0) return sn::fail(SN_ERR_INVALID_ARG, "%s: B must be positive (got %d)", what, B);
    if (nx <= 0 || ny <= 0 || nz <= 0)
        return sn::fail(SN_ERR_INVALID_ARG, "%s: non-positive grid extent (%d, %d, %d)", what, nx, ny, nz);
    if (total > kMaxTotal)
        return sn::fail(SN_ERR_UNSUPPORTED, "%s: total=%lld >= 2^31 (a count must fit int32, a sum int64)", what, (long long)total);
    if (B > kMaxB) return sn::fail(SN_ERR_UNSUPPORTED, "%s: B=%d beyond what is served (B <= %d)", what, B, kMaxB);
    const size_t lds = ((size_t)nx + (size_t)ny + (size_t)nz + 3) * sizeof(double);
    if (lds > 64 * 1024 - 2 * kMaxP * sizeof(double))
        return sn::fail(SN_ERR_UNSUPPORTED, "%s: edge tables beyond 64 KiB of LDS", what);
    const int64_t V = (int64_t)nx * ny * nz;
    if (V >= ((int64_t)1 << 31)) return sn::fail(SN_ERR_UNSUPPORTED, "%s: nx * ny * nz >= 2^31", what);
    if ((uintptr_t)pts % 8 || (uintptr_t)values % 8 || (uintptr_t)offsets % 8 || (uintptr_t)desc % 8 ||
        (uintptr_t)out % 8 || (uintptr_t)unbinned % 8 || (uintptr_t)nan_rows % 8 || (uintptr_t)counts % 4)
        return sn::fail(SN_ERR_INVALID_ARG,
                        "%s: pts / values / offsets / desc / out / unbinned / nan_rows must be 8-byte, counts 4-byte aligned",
                        what);
    (void)ws;   // no workspace is needed: sn_voxel_pool_ws_bytes is 0
    hipStream_t s = sn::as_stream(stream);
    unsigned long long* o = reinterpret_cast<unsigned long long*>(out);
    unsigned long long* u = reinterpret_cast<unsigned long long*>(unbinned);
    unsigned long long* n = reinterpret_cast<unsigned long long*>(nan_rows);
    const int desc_len = 6 + nx + ny + nz + 3;
    // a launch's x walks one plane's cells, its y the (tile, plane) pairs
    const auto cover = [](int64_t cells, int64_t rows) {
        const int64_t want = (cells + 256 * 4 - 1) / (256 * 4);
        const int64_t gx = want < 2048 ? (want > 0 ? want : 1) : 2048;
        const int64_t gy = rows < 8192 / gx ? rows : (8192 / gx > 0 ? 8192 / gx : 1);
        return dim3((unsigned)gx, (unsigned)gy);
    };
    const dim3 rows_grid((unsigned)((total + kWaveChunk - 1) / kWaveChunk)), wave(kWaveLanes);
    hipLaunchKernelGGL(pool_clear_kernel, cover(V, (int64_t)B * (P + 1)), dim3(256), 0, s, plan, B, V, o, counts, u, n);
    if (flags & SN_VOXEL_POOL_NO_LOOK)
        hipLaunchKernelGGL(pool_rows_kernel<false>, rows_grid, wave, lds, s, plan, pts, values, offsets, total, B, desc, nx, ny,
                           nz, o, counts, u, n);
    else
        hipLaunchKernelGGL(pool_rows_kernel<true>, rows_grid, wave, lds, s, plan, pts, values, offsets, total, B, desc, nx, ny,
                           nz, o, counts, u, n);
    hipLaunchKernelGGL(pool_decode_kernel, cover(V, (int64_t)B * P), dim3(256), 0, s, plan, B, V, desc, desc_len, o, counts);
    return sn::check_launch(what);
}
