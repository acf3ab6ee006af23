// K16 -- coloured voxel clouds: the non-zero voxels of B grids compacted into rows (x, y, z, r, g, b), a CSR batch of B
// clouds (sn_voxel_cloud_count, sn_voxel_cloud_scatter).
// replaces: the data half of plot_voxelgrid (utils/voxelization.py:45-144) with color_pointcloud
//           (utils/pcd_processing.py:525-574) behind it -- a Python loop over grid.nonzero() and an np.where per voxel, on
//           the host, after a .detach().cpu().numpy() of every logged grid (core/lit_modules/lit_model_wrappers.py:222-233).
//
// Definition (normative, include/scenenet_hip.h).  A grid is [n0, n1, n2] = [Z, X, Y]; a voxel value is read as fp64 (an
// f32 widens exactly).  density: a cell is live iff value != 0 (-0.0 is zero, NaN is not); its colour is
// c < 0 ? (1 + c, 1 + c, 1) : (1, 1 - c, 1 - c), each sum rounded once, then times 255.0, rounded once (this file is built
// with -ffp-contract=off).  ranges: a cell is live iff value > lin[1]; its colour is row argmin_j |(value - lin[j]) - step|
// of the table (the first minimum wins), times 255.0.  Cloud b holds tile b's live cells in C order of (z, x, y).
//
// Shape: crops.hip's, its scans and ranks from scan.h.  One WAVE per workgroup and kWaveChunk = 1024 consecutive cells of one
// tile per workgroup; lane l looks at the cells chunk * 1024 + g * 64 + l, g = 0..15.  Per group __ballot of the live test gives the wave-uniform __popcll
// (count) and, in the scatter, the lane's rank by mbcnt of the same mask: output order is cell order by construction.
//   count:   ws[b][chunk] = live cells of the chunk, and two slots per chunk for `bad` (one slot per workgroup each: no
//            memset, no atomics)
//   prefix:  one workgroup per tile turns its row into exclusive prefixes, total in ws[b][nchunks]; sums the bad slots
//   offsets: one workgroup, the exclusive prefix of the totals
//   scatter: recomputes the test (a chunk whose count is zero leaves at once), forms the row and stores it: 48 B as three
//            16-byte stores per lane, a wave's rows contiguous in the output.
//
// Bound: the count reads the grid once (1..8 B per cell), the scatter once more and writes 48 B per live cell (24 + 6 in
// the xyz / rgb16 form).  The index split costs two 32-bit divisions per cell and pass; nothing else is more than a dozen
// VALU operations per cell in `density`, 7 r per live cell in `ranges`.  HBM-bound by design.
#include <cfloat>
#include "common.h"
#include "scan.h"

namespace {

using sn::kWaveLanes;     // scan.h: kWaveGroups groups of 64 consecutive cells, kWaveChunk cells per workgroup
using sn::kWaveGroups;
using sn::kWaveChunk;
using sn::kScanThreads;
using sn::kScanItems;
constexpr int kMaxB = 65535;                 // (tiles are the launch grid's y)
constexpr int64_t kMaxV = ((int64_t)1 << 31) - 1;   // cells per tile: the index split is 32-bit
constexpr int kMaxR = 32;

struct CloudParams {
    double lin[kMaxR];         // np.linspace(0, 1, r)
    double tab[kMaxR * 3];     // 255.0 * colour table rows
    double step;               // (1 / r) / 2
    int r, mode;
};

template <typename T> __device__ __forceinline__ double widen(T v) { return (double)v; }

__device__ __forceinline__ bool is_live(double v, int mode, double lin1) {
    return mode == SN_CLOUD_RANGES ? v > lin1 : v != 0.0;   // (NaN != 0 is true, NaN > lin1 false; -0.0 != 0 false)
}

// 255 * the density colour's varying channel (the other is 255 or sits beside it twice): c < 0 ? 1 + c : 1 - c
__device__ __forceinline__ double density_channel(double c) {
#pragma clang fp contract(off)
    const double ch = c < 0.0 ? 1.0 + c : 1.0 - c;
    return ch * 255.0;
}

// The tables travel in the kernel's arguments, which live in scalar registers: an index held per lane would send the whole
// struct to scratch.  The wave copies them into LDS once (every index into P a compile-time constant, the loop left by a
// wave-uniform branch at r) and walks lin there: the same address in every lane, a broadcast read.
__device__ __forceinline__ void stage_tables(const CloudParams& P, int lane, double* s_lin, double* s_tab) {
    double l = 0.0, t0 = 0.0, t1 = 0.0, t2 = 0.0;
#pragma unroll
    for (int j = 0; j < kMaxR; ++j) {
        if (j >= P.r) break;
        const bool mine = lane == j;
        l = mine ? P.lin[j] : l;
        t0 = mine ? P.tab[3 * j] : t0;
        t1 = mine ? P.tab[3 * j + 1] : t1;
        t2 = mine ? P.tab[3 * j + 2] : t2;
    }
    if (lane < kMaxR) {
        s_lin[lane] = l;
        s_tab[3 * lane] = t0;
        s_tab[3 * lane + 1] = t1;
        s_tab[3 * lane + 2] = t2;
    }
    __syncthreads();
}
__device__ __forceinline__ int ranges_row(double v, const double* s_lin, double step, int r) {
#pragma clang fp contract(off)
    int best = 0;
    double dbest = fabs((v - s_lin[0]) - step);
    for (int j = 1; j < r; ++j) {
        const double d = fabs((v - s_lin[j]) - step);
        const bool better = d < dbest;   // (strict: the first minimum wins, as np.argmin has it)
        dbest = better ? d : dbest;
        best = better ? j : best;
    }
    return best;
}

struct Split { int i0, i1, i2; };
__device__ __forceinline__ Split split(uint32_t n, uint32_t n1, uint32_t n2) {
    const uint32_t i01 = n / n2;
    Split s;
    s.i2 = (int)(n - i01 * n2);
    s.i0 = (int)(i01 / n1);
    s.i1 = (int)(i01 - (uint32_t)s.i0 * n1);
    return s;
}

// a size-mode descriptor pads its edge tables with +inf beyond the tile's own dims: such a cell is not part of the tile's
// grid (gather_points_kernel's rule).  d: the tile's descriptor; [Z, X, Y] = [n0, n1, n2], edges of x, y, z in this order
__device__ __forceinline__ bool cell_in_tile(const double* __restrict__ d, const Split& s, int n1, int n2) {
    const double *ex = d + 6, *ey = ex + n1 + 1, *ez = ey + n2 + 1;
    return ex[s.i1 + 1] <= DBL_MAX && ey[s.i2 + 1] <= DBL_MAX && ez[s.i0 + 1] <= DBL_MAX;
}
__device__ __forceinline__ bool tile_padded(const double* __restrict__ d, int n0, int n1, int n2) {
    const double *ex = d + 6, *ey = ex + n1 + 1, *ez = ey + n2 + 1;
    return !(ex[n1] <= DBL_MAX && ey[n2] <= DBL_MAX && ez[n0] <= DBL_MAX);
}

// ws of tile b: [0 .. nchunks] counts -> prefixes and the total, then (nan, colour) slots per chunk
__host__ __device__ __forceinline__ int64_t ws_stride(int64_t nchunks) { return 3 * nchunks + 1; }

template <typename T>
__global__ __launch_bounds__(kWaveLanes) void cloud_count_kernel(const T* __restrict__ grid, int64_t V, int n0, int n1, int n2,
                                                             int mode, double lin1, const double* __restrict__ desc,
                                                             int desc_len, int64_t nchunks, int64_t* __restrict__ ws) {
    const int lane = threadIdx.x;
    const int64_t chunk = blockIdx.x;
    const int b = blockIdx.y;
    const T* g = grid + (int64_t)b * V;
    const double* d = desc ? desc + (int64_t)b * desc_len : nullptr;
    const bool padded = d && tile_padded(d, n0, n1, n2);
    int cnt = 0, cnan = 0, ccol = 0;
#pragma unroll
    for (int q = 0; q < kWaveGroups; ++q) {
        const int64_t n = chunk * kWaveChunk + q * kWaveLanes + lane;
        const double v = n < V ? widen(g[n]) : 0.0;
        bool live = is_live(v, mode, lin1);       // (past the end: 0.0, live in neither mode -- lin1 > 0)
        if (padded && live) live = cell_in_tile(d, split((uint32_t)n, (uint32_t)n1, (uint32_t)n2), n1, n2);
        cnt += __popcll(__ballot(live));
        if (mode == SN_CLOUD_DENSITY) {
            const bool nan = v != v;
            const double t = density_channel(v);
            cnan += __popcll(__ballot(live && nan));
            ccol += __popcll(__ballot(live && !nan && (t < 0.0 || t > 255.0)));
        }
    }
    if (lane == 0) {
        int64_t* row = ws + (int64_t)b * ws_stride(nchunks);
        row[chunk] = cnt;
        row[nchunks + 1 + 2 * chunk] = cnan;
        row[nchunks + 2 + 2 * chunk] = ccol;
    }
}

// workgroup b: ws[b][0 .. nchunks) counts -> exclusive prefixes, ws[b][nchunks] = the tile's total; bad[b] = the sums of
// the chunks' slots (integers: the order of the additions is fixed and would not matter)
__global__ __launch_bounds__(kScanThreads) void cloud_prefix_kernel(int64_t* __restrict__ ws, int64_t nchunks,
                                                                    int64_t* __restrict__ bad) {
    __shared__ int64_t s_wave[kScanThreads / 64];
    int64_t* row = ws + (int64_t)blockIdx.x * ws_stride(nchunks);
    const int64_t live = sn::scan_row<kScanThreads, kScanItems>(row, nchunks, s_wave);
    if (threadIdx.x == 0) row[nchunks] = live;
    // thread t sums the slots t, t + 256, ... of each kind; the block sums the threads
    const int64_t* slots = row + nchunks + 1;
    int64_t a[2] = {0, 0};
    for (int64_t c = threadIdx.x; c < nchunks; c += kScanThreads) {
        a[0] += slots[2 * c];
        a[1] += slots[2 * c + 1];
    }
    for (int k = 0; k < 2; ++k) {
        int64_t v[1] = {a[k]};
        const int64_t total = sn::block_exclusive<kScanThreads, 1>(v, s_wave);
        if (threadIdx.x == 0) bad[2 * (int64_t)blockIdx.x + k] = total;
    }
}

// one workgroup: offsets[b] = live cells of the tiles before b, offsets[B] = all
__global__ __launch_bounds__(kScanThreads) void cloud_offsets_kernel(const int64_t* __restrict__ ws, int64_t nchunks, int B,
                                                                     int64_t* __restrict__ offsets) {
    __shared__ int64_t s_wave[kScanThreads / 64];
    sn::totals_to_offsets<kScanThreads>(ws, ws_stride(nchunks), nchunks, B, offsets, s_wave);
}

// NaN -> 0
__device__ __forceinline__ uint16_t rgb16_of(double t) {
    double r = rint(t);
    r = r < 0.0 ? 0.0 : (r > 255.0 ? 255.0 : r);
    return t != t ? (uint16_t)0 : (uint16_t)((int)r * 257);
}

template <typename T, bool kRanges>
__global__ __launch_bounds__(kWaveLanes) void cloud_scatter_kernel(const T* __restrict__ grid, int64_t V, int n0, int n1, int n2,
                                                               CloudParams P, const double* __restrict__ desc, int desc_len,
                                                               int64_t nchunks, const int64_t* __restrict__ ws,
                                                               const int64_t* __restrict__ offsets, int64_t capacity,
                                                               double* __restrict__ rows, double* __restrict__ xyz,
                                                               uint16_t* __restrict__ rgb16) {
    const int lane = threadIdx.x;
    const int64_t chunk = blockIdx.x;
    const int b = blockIdx.y;
    const int64_t* slot = ws + (int64_t)b * ws_stride(nchunks) + chunk;
    const int64_t before = slot[0];
    if (slot[1] == before) return;     // no live cell in this chunk, by the count pass's own test (slot[1] of the last
                                       // chunk is the tile's total)
    int64_t row = offsets[b] + before;
    const T* g = grid + (int64_t)b * V;
    const double* d = desc ? desc + (int64_t)b * desc_len : nullptr;
    const bool padded = d && tile_padded(d, n0, n1, n2);
    const double lin1 = P.lin[1];
    constexpr int kMode = kRanges ? SN_CLOUD_RANGES : SN_CLOUD_DENSITY;
    __shared__ double s_lin[kRanges ? kMaxR : 1], s_tab[kRanges ? kMaxR * 3 : 1];
    if (kRanges) stage_tables(P, lane, s_lin, s_tab);   // (behind the wave-uniform return above: one wave, nobody waits)
#pragma unroll
    for (int q = 0; q < kWaveGroups; ++q) {
        const int64_t n = chunk * kWaveChunk + q * kWaveLanes + lane;
        const double v = n < V ? widen(g[n]) : 0.0;
        bool live = is_live(v, kMode, lin1);
        Split s{0, 0, 0};
        if (live) {
            s = split((uint32_t)n, (uint32_t)n1, (uint32_t)n2);
            if (padded) live = cell_in_tile(d, s, n1, n2);
        }
        const unsigned long long mask = __ballot(live);
        if (live) {
            const int64_t o = row + sn::wave_rank(mask);
            if ((uint64_t)o < (uint64_t)capacity) {   // (also keeps a workspace that is not this call's inside the buffers)
                double x, y, z, cr, cg, cb;
                if (d) {
                    const double *ex = d + 6, *ey = ex + n1 + 1, *ez = ey + n2 + 1;
                    x = (ex[s.i1] + ex[s.i1 + 1]) * 0.5;
                    y = (ey[s.i2] + ey[s.i2 + 1]) * 0.5;
                    z = (ez[s.i0] + ez[s.i0 + 1]) * 0.5;
                } else {
                    x = (double)s.i1;
                    y = (double)s.i2;
                    z = (double)s.i0;
                }
                if (kRanges) {
                    const double* t = s_tab + 3 * ranges_row(v, s_lin, P.step, P.r);
                    cr = t[0];
                    cg = t[1];
                    cb = t[2];
                } else {
                    const double t = density_channel(v);
                    const bool neg = v < 0.0;
                    cr = neg ? t : 255.0;
                    cg = t;
                    cb = neg ? 255.0 : t;
                }
                if (rows) {
                    double2* p = reinterpret_cast<double2*>(rows + o * 6);
                    p[0] = make_double2(x, y);
                    p[1] = make_double2(z, cr);
                    p[2] = make_double2(cg, cb);
                }
                if (xyz) {
                    double* p = xyz + o * 3;
                    p[0] = x;
                    p[1] = y;
                    p[2] = z;
                }
                if (rgb16) {
                    uint16_t* p = rgb16 + o * 3;
                    p[0] = rgb16_of(cr);
                    p[1] = rgb16_of(cg);
                    p[2] = rgb16_of(cb);
                }
            }
        }
        row += __popcll(mask);
    }
}

int64_t host_nchunks(int64_t V) { return (V + kWaveChunk - 1) / kWaveChunk; }
bool shape_served(int B, int64_t V) { return B > 0 && V > 0 && B <= kMaxB && V <= kMaxV; }

size_t dtype_size(int dtype) {
    switch (dtype) {
        case SN_F32: return 4;
        case SN_F64: return 8;
        case SN_U8:
        case SN_OCC8: return 1;
        default: return 0;
    }
}

// the checks both entries share; `what` names the entry in the error text
int check_common(const char* what, const void* grid, int dtype, int B, int n0, int n1, int n2, int mode, int r,
                 const void* desc, const void* ws, size_t ws_bytes, const void* offsets) {
    if (!grid) return sn::fail(SN_ERR_INVALID_ARG, "%s: grid is null", what);
    if (!ws) return sn::fail(SN_ERR_INVALID_ARG, "%s: ws is null", what);
    if (!offsets) return sn::fail(SN_ERR_INVALID_ARG, "%s: offsets is null", what);
    if (B <= 0) return sn::fail(SN_ERR_INVALID_ARG, "%s: B must be positive (got %d)", what, B);
    if (n0 <= 0 || n1 <= 0 || n2 <= 0)
        return sn::fail(SN_ERR_INVALID_ARG, "%s: the extents must be positive (got %d x %d x %d)", what, n0, n1, n2);
    if (mode != SN_CLOUD_DENSITY && mode != SN_CLOUD_RANGES)
        return sn::fail(SN_ERR_INVALID_ARG, "%s: unknown mode %d (SN_CLOUD_DENSITY | SN_CLOUD_RANGES)", what, mode);
    if (mode == SN_CLOUD_RANGES && (r < 2 || r > kMaxR))
        return sn::fail(SN_ERR_INVALID_ARG, "%s: r=%d is outside 2..%d", what, r, kMaxR);
    const size_t esz = dtype_size(dtype);
    if (esz == 0)
        return sn::fail(SN_ERR_INVALID_ARG, "%s: grid dtype %d not accepted (SN_F32 | SN_F64 | SN_U8 | SN_OCC8)", what, dtype);
    const int64_t V = (int64_t)n0 * n1 * n2;
    if (!shape_served(B, V))
        return sn::fail(SN_ERR_UNSUPPORTED, "%s: B=%d tiles of %lld cells beyond what is served (B <= %d, cells < 2^31)", what,
                        B, (long long)V, kMaxB);
    if (ws_bytes < sn_voxel_cloud_ws_bytes(B, V))
        return sn::fail(SN_ERR_INVALID_ARG, "%s: workspace of %zu bytes, sn_voxel_cloud_ws_bytes asks for %zu", what, ws_bytes,
                        sn_voxel_cloud_ws_bytes(B, V));
    if ((uintptr_t)grid % esz || (uintptr_t)desc % 8 || (uintptr_t)ws % 8 || (uintptr_t)offsets % 8)
        return sn::fail(SN_ERR_INVALID_ARG, "%s: grid must be element-aligned, desc / ws / offsets 8-byte aligned", what);
    return SN_OK;
}

// np.linspace(0, 1, r) as numpy forms it: arange(r) * (1 / (r - 1)) + 0, the last entry set to 1
void fill_lin(CloudParams& P, int mode, int r) {
    P.mode = mode;
    P.r = mode == SN_CLOUD_RANGES ? r : 2;
    const double step = 1.0 / (double)(P.r - 1);
    for (int j = 0; j < kMaxR; ++j) P.lin[j] = j < P.r ? (double)j * step + 0.0 : 0.0;
    P.lin[P.r - 1] = 1.0;
    P.step = (1.0 / (double)P.r) / 2.0;
}

}  // namespace

extern "C" int sn_voxel_cloud_chunk_cells(void) { return kWaveChunk; }

extern "C" size_t sn_voxel_cloud_ws_bytes(int B, int64_t V) {
    if (!shape_served(B, V)) return 0;
    return (size_t)B * (size_t)ws_stride(host_nchunks(V)) * sizeof(int64_t);
}

extern "C" int sn_voxel_cloud_count(const void* grid, int dtype, int B, int n0, int n1, int n2, int mode, int r,
                                    const double* desc, void* ws, size_t ws_bytes, int64_t* offsets, int64_t* bad,
                                    sn_stream_t stream) {
    const char* what = "sn_voxel_cloud_count";
    const int rc = check_common(what, grid, dtype, B, n0, n1, n2, mode, r, desc, ws, ws_bytes, offsets);
    if (rc != SN_OK) return rc;
    if (!bad) return sn::fail(SN_ERR_INVALID_ARG, "%s: bad is null", what);
    if ((uintptr_t)bad % 8) return sn::fail(SN_ERR_INVALID_ARG, "%s: bad must be 8-byte aligned", what);
    CloudParams P;
    fill_lin(P, mode, r);
    hipStream_t s = sn::as_stream(stream);
    const int64_t V = (int64_t)n0 * n1 * n2, nchunks = host_nchunks(V);
    const int dlen = SN_DESC_LEN(n1, n2, n0);
    int64_t* w = static_cast<int64_t*>(ws);
    const dim3 grd((unsigned)nchunks, (unsigned)B);
#define SN_COUNT(T)                                                                                                    \
    hipLaunchKernelGGL(cloud_count_kernel<T>, grd, dim3(kWaveLanes), 0, s, static_cast<const T*>(grid), V, n0, n1, n2, mode, \
                       P.lin[1], desc, dlen, nchunks, w)
    switch (dtype) {
        case SN_F32: SN_COUNT(float); break;
        case SN_F64: SN_COUNT(double); break;
        default: SN_COUNT(uint8_t); break;
    }
#undef SN_COUNT
    hipLaunchKernelGGL(cloud_prefix_kernel, dim3((unsigned)B), dim3(kScanThreads), 0, s, w, nchunks, bad);
    hipLaunchKernelGGL(cloud_offsets_kernel, dim3(1), dim3(kScanThreads), 0, s, w, nchunks, B, offsets);
    return sn::check_launch(what);
}

extern "C" int sn_voxel_cloud_scatter(const void* grid, int dtype, int B, int n0, int n1, int n2, int mode, int r,
                                      const double* table_host, const double* desc, const void* ws, size_t ws_bytes,
                                      const int64_t* offsets, int64_t capacity, double* rows, double* xyz, uint16_t* rgb16,
                                      sn_stream_t stream) {
    const char* what = "sn_voxel_cloud_scatter";
    const int rc = check_common(what, grid, dtype, B, n0, n1, n2, mode, r, desc, ws, ws_bytes, offsets);
    if (rc != SN_OK) return rc;
    if (mode == SN_CLOUD_RANGES && !table_host) return sn::fail(SN_ERR_INVALID_ARG, "%s: table_host is null (ranges)", what);
    if (!rows && !xyz) return sn::fail(SN_ERR_INVALID_ARG, "%s: neither rows nor xyz is given", what);
    if (capacity < 0)
        return sn::fail(SN_ERR_INVALID_ARG, "%s: capacity must not be negative (got %lld)", what, (long long)capacity);
    if ((uintptr_t)rows % 16 || (uintptr_t)xyz % 8 || (uintptr_t)rgb16 % 2)
        return sn::fail(SN_ERR_INVALID_ARG, "%s: rows must be 16-byte, xyz 8-byte, rgb16 2-byte aligned", what);
    CloudParams P;
    fill_lin(P, mode, r);
    for (int j = 0; j < kMaxR * 3; ++j)
        P.tab[j] = (mode == SN_CLOUD_RANGES && j < 3 * r) ? table_host[j] * 255.0 : 0.0;
    const int64_t V = (int64_t)n0 * n1 * n2, nchunks = host_nchunks(V);
    const int dlen = SN_DESC_LEN(n1, n2, n0);
    const dim3 grd((unsigned)nchunks, (unsigned)B);
#define SN_SCATTER_M(T, M)                                                                                           \
    hipLaunchKernelGGL((cloud_scatter_kernel<T, M>), grd, dim3(kWaveLanes), 0, sn::as_stream(stream),                       \
                       static_cast<const T*>(grid), V, n0, n1, n2, P, desc, dlen, nchunks, static_cast<const int64_t*>(ws), \
                       offsets, capacity, rows, xyz, rgb16)
#define SN_SCATTER(T)                                                     \
    do {                                                                  \
        if (mode == SN_CLOUD_RANGES) SN_SCATTER_M(T, true);               \
        else SN_SCATTER_M(T, false);                                      \
    } while (0)
    switch (dtype) {
        case SN_F32: SN_SCATTER(float); break;
        case SN_F64: SN_SCATTER(double); break;
        default: SN_SCATTER(uint8_t); break;
    }
#undef SN_SCATTER
#undef SN_SCATTER_M
    return sn::check_launch(what);
}
