// K18 -- semantic voxel grids and class colours: the largest label of every voxel of a CSR batch (sn_voxel_classes), the
// set of classes of every tile (sn_class_census) and each point's colour by its class's rank in that set (sn_class_paint).
// replaces: classes_on_voxel (utils/voxelization.py:207-241): a pandas DataFrame of (label, z, x, y), groupby(["z", "x",
//           "y"]).max() and a Python loop over the occupied voxels into np.zeros; and color_pointcloud
//           (utils/pcd_processing.py:525-574): np.unique(classes), then a Python loop over EVERY point with
//           class_color[np.where(unique_classes == c)[0][0]] inside it.
//
// Definition (normative, include/scenenet_hip.h).  Grid: a row is binned by sn::Binner::flat (binning.h: the text voxel.hip
// and thin.hip bin with); a voxel no binned row falls in holds +0.0, one whose binned rows all carry NaN labels holds NaN,
// any other the largest label that is not NaN.  Colours: rank(c) = the number of distinct valid classes of the tile below
// c; the row's colour is table[rank].
//
// Shape, grid: thin.hip's -- one WAVE per workgroup, kWaveChunk = 1024 consecutive rows of the packed batch, the tiles that
// reach into the chunk walked (sn::for_tiles, packed_rows.h; census and paint walk their chunks with it too) one edge table
// in LDS at a time.  A label becomes the order-preserving key of common.h (enc_f64): every key of a value that is not NaN
// is >= 0x000FFFFFFFFFFFFF (-inf), which leaves 0 for "empty" and 1 for "NaN labels only".  The keys live in the grid's
// own cells:
//   zero      grid, unbinned, nan_labels <- 0 (one kernel, no memset node: see zero_kernel)
//   points    one 64-bit integer atomic max per binned row, sent only where a plain load of the cell shows less than the
//             row's key (the cell only grows: a stale look costs a needless atomic, never a result)
//   decode    the grid in place: 0 -> +0.0, 1 -> NaN, any other key -> its label
// A maximum of integers: the result does not depend on scheduling.
//
// Shape, colours: 256 threads per workgroup, kClassChunk = 8192 consecutive rows, row base + k * 256 + thread for k = 0..31.
//   census    per tile in the chunk: a bitmap of 65536 bits in LDS (set by LDS atomic OR where a look shows the bit
//             clear), merged into present[b] by 32-bit atomic OR of the words that are not zero
//   unique    workgroup b: popcounts of present[b], their exclusive prefix (scan.h) -> n_unique[b], unique[b][..],
//             short_table[b] <- 0
//   paint     per tile in the chunk: present[b] and the prefix of its words into LDS (scan.h), then per row
//             rank = prefix[c >> 5] + popcount(word & below bit), the table's row as three 64-bit patterns
//
// Bound: the grid reads 32 B per row and writes 8 B per cell three times over (zeroing, atomics' lines, decode); census
// reads 8 B per row; paint reads 8 B and writes 24 B (colors) and / or 6 B (rgb) per row.
#include "common.h"
#include "binning.h"
#include "packed_rows.h"
#include "scan.h"

namespace {

using sn::kWaveLanes;
using sn::kWaveGroups;
using sn::kWaveChunk;
constexpr int kMaxB = 1 << 16;
constexpr int64_t kMaxTotal = (int64_t)1 << 33;
constexpr unsigned long long kKeyEmpty = 0ull, kKeyNan = 1ull;
constexpr uint64_t kNanBits = 0x7ff8000000000000ull;

constexpr int kClassThreads = 256;
constexpr int kClassRounds = 32;
constexpr int kClassChunk = kClassThreads * kClassRounds;   // rows per workgroup of census and paint
constexpr int kClassWords = SN_CLASS_WORDS;                 // 65536 bits
constexpr int kClassItems = kClassWords / kClassThreads;    // words per thread of a prefix
constexpr int kClassBatch = 8;                              // rows per thread whose loads are in flight together
static_assert(kClassRounds % kClassBatch == 0, "whole batches");
static_assert(kClassItems * kClassThreads == kClassWords, "one scan tile holds the bitmap");

// p[0 .. n) <- 0 (the grid's keys, a tile's bitmap) and c0[0 .. m), c1[0 .. m) <- 0 (the per-tile counters the kernels
// behind it add into; c1 nullable), in one launch.  A kernel, not memset nodes: [measured] with several memset nodes in one
// captured graph, the second one (16 bytes in one run, 16 KiB in another) left address-like words in its target from the
// second replay on, an eager call on the same buffers in between.
template <typename T>
__global__ __launch_bounds__(256) void zero_kernel(T* __restrict__ p, int64_t n, unsigned long long* __restrict__ c0,
                                                   unsigned long long* __restrict__ c1, int m) {
    const int64_t stride = (int64_t)gridDim.x * 256, first = (int64_t)blockIdx.x * 256 + threadIdx.x;
    for (int64_t i = first; i < n; i += stride) p[i] = (T)0;
    for (int64_t i = first; i < m; i += stride) {
        c0[i] = 0ull;
        if (c1) c1[i] = 0ull;
    }
}
template <typename T>
void zero(T* p, int64_t n, unsigned long long* c0, unsigned long long* c1, int m, hipStream_t s) {
    const int64_t want = (n + 256 * 4 - 1) / (256 * 4);
    hipLaunchKernelGGL(zero_kernel<T>, dim3((unsigned)(want < 8192 ? want : 8192)), dim3(256), 0, s, p, n, c0, c1, m);
}

// ---------------------------------------------------------------- the class grid
template <bool kSkip>
__global__ __launch_bounds__(kWaveLanes) void classes_points_kernel(const double* __restrict__ pts,
                                                                    const double* __restrict__ labels,
                                                                    const int64_t* __restrict__ offsets, int64_t total, int B,
                                                                    const double* __restrict__ desc, int nx, int ny, int nz,
                                                                    unsigned long long* __restrict__ grid,
                                                                    unsigned long long* __restrict__ unbinned,
                                                                    unsigned long long* __restrict__ nan_labels) {
    extern __shared__ double edges[];
    const int lane = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * kWaveChunk;
    const int ne = nx + ny + nz + 3;
    const int64_t V = (int64_t)nx * ny * nz;
    sn::for_tiles(offsets, B, base, kWaveChunk, total, [&](int b, int64_t, int64_t, int64_t from, int64_t to) {
        const double* d = desc + (size_t)b * (size_t)(6 + ne);
        __syncthreads();   // the previous tile's table has been read
        sn::load_edges(edges, d, ne, kWaveLanes);
        sn::Binner bin;
        bin.init(edges, d, nx, ny, nz);
        unsigned long long* cells = grid + (size_t)b * (size_t)V;
        int nunb = 0, nnan = 0;
#pragma unroll 4
        for (int g = 0; g < kWaveGroups; ++g) {
            const int64_t i = base + g * kWaveLanes + lane;
            const bool mine = i >= from && i < to;
            bool unb = false, isnan = false;
            if (mine) {
                const double* p = pts + i * 3;
                const double lab = labels[i];
                const int f = bin.flat(p[0], p[1], p[2]);
                isnan = lab != lab;
                unb = f < 0;
                if (!unb) {
                    const unsigned long long key = isnan ? kKeyNan : sn::enc_f64(lab);
                    unsigned long long* cell = cells + f;
                    if (!kSkip || __hip_atomic_load(cell, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < key)
                        __hip_atomic_fetch_max(cell, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
            nunb += __popcll(__ballot(unb));
            nnan += __popcll(__ballot(isnan));
        }
        if (lane == 0) {
            if (nunb) __hip_atomic_fetch_add(unbinned + b, (unsigned long long)nunb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (nnan) __hip_atomic_fetch_add(nan_labels + b, (unsigned long long)nnan, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    });
}

// keys -> labels, in place
__global__ __launch_bounds__(256) void classes_decode_kernel(unsigned long long* __restrict__ grid, int64_t cells) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < cells; i += stride) {
        const unsigned long long k = grid[i];
        unsigned long long v;
        if (k == kKeyEmpty) v = 0ull;
        else if (k == kKeyNan) v = kNanBits;
        else v = (unsigned long long)__double_as_longlong(sn::dec_f64(k));
        grid[i] = v;
    }
}

// ---------------------------------------------------------------- class colours
// the class of a valid value (integral, 0 .. 65535), -1 for every other (NaN fails both comparisons)
__device__ __forceinline__ int class_of(double c) {
    if (!(c >= 0.0 && c <= 65535.0)) return -1;
    const int k = (int)c;
    return (double)k == c ? k : -1;
}

__global__ __launch_bounds__(kClassThreads) void class_census_kernel(const double* __restrict__ classes,
                                                                    const int64_t* __restrict__ offsets, int64_t total, int B,
                                                                    uint32_t* __restrict__ present,
                                                                    unsigned long long* __restrict__ bad) {
    __shared__ uint32_t s_bits[kClassWords];
    const int t = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * kClassChunk;
    sn::for_tiles(offsets, B, base, kClassChunk, total, [&](int b, int64_t, int64_t, int64_t from, int64_t to) {
        __syncthreads();   // the previous tile's bitmap has been merged
        for (int w = t; w < kClassWords; w += kClassThreads) s_bits[w] = 0u;
        __syncthreads();
        // kClassBatch rows per thread are loaded before the first is looked at: the loads of a batch are in flight together
        int nbad = 0;
        const int first = (int)((from - base) / kClassThreads), last = (int)((to - 1 - base) / kClassThreads);
        for (int k0 = first; k0 <= last; k0 += kClassBatch) {
            double v[kClassBatch];
            bool in[kClassBatch];
#pragma unroll
            for (int q = 0; q < kClassBatch; ++q) {
                const int64_t i = base + (int64_t)(k0 + q) * kClassThreads + t;   // (rounds behind `last` are at or behind `to`)
                in[q] = i >= from && i < to;
                v[q] = in[q] ? classes[i] : 0.0;
            }
#pragma unroll
            for (int q = 0; q < kClassBatch; ++q) {
                const int c = class_of(v[q]);
                if (in[q] && c >= 0) {
                    const uint32_t m = 1u << (c & 31);
                    if (!(s_bits[c >> 5] & m))
                        __hip_atomic_fetch_or(&s_bits[c >> 5], m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                }
                nbad += in[q] && c < 0;
            }
        }
        nbad = sn::wave_reduce(nbad, [](int a, int b) { return a + b; });
        if ((t & 63) == 0 && nbad)
            __hip_atomic_fetch_add(bad + b, (unsigned long long)nbad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __syncthreads();
        uint32_t* mine = present + (size_t)b * kClassWords;
        for (int w = t; w < kClassWords; w += kClassThreads) {
            const uint32_t v = s_bits[w];
            if (v) __hip_atomic_fetch_or(mine + w, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    });
}

// thread t's kClassItems consecutive words of a tile's bitmap and the exclusive prefix of their popcounts; returns the
// tile's number of classes.  s_wave: kClassThreads / 64 slots
__device__ __forceinline__ int words_and_prefix(const uint32_t* __restrict__ mine, uint32_t (&w)[kClassItems],
                                                int (&pre)[kClassItems], int* s_wave) {
    const int t = threadIdx.x;
#pragma unroll
    for (int q = 0; q < kClassItems; ++q) {
        w[q] = mine[t * kClassItems + q];
        pre[q] = __popc(w[q]);
    }
    return sn::block_exclusive<kClassThreads, kClassItems, int>(pre, s_wave);
}

// workgroup b: n_unique[b], unique[b][0 .. min(n_unique, U_max)), short_table[b] <- 0
__global__ __launch_bounds__(kClassThreads) void class_unique_kernel(const uint32_t* __restrict__ present, double* __restrict__ unique,
                                                                    int U_max, int64_t* __restrict__ n_unique,
                                                                    int64_t* __restrict__ short_table) {
    __shared__ int s_wave[kClassThreads / 64];
    const int b = blockIdx.x, t = threadIdx.x;
    uint32_t w[kClassItems];
    int pre[kClassItems];
    const int n = words_and_prefix(present + (size_t)b * kClassWords, w, pre, s_wave);
    if (t == 0) {
        n_unique[b] = n;
        short_table[b] = 0;
    }
    if (!unique) return;
    double* out = unique + (size_t)b * (size_t)U_max;
#pragma unroll
    for (int q = 0; q < kClassItems; ++q) {
        uint32_t bits = w[q];
        int o = pre[q];
        while (bits) {
            const int bit = __ffs((int)bits) - 1;
            bits &= bits - 1u;
            if (o < U_max) out[o] = (double)((t * kClassItems + q) * 32 + bit);
            ++o;
        }
    }
}

// NaN -> 0
__device__ __forceinline__ uint16_t rgb16_of(double c) {
    const double t = 255.0 * c;
    double r = rint(t);
    r = r < 0.0 ? 0.0 : (r > 255.0 ? 255.0 : r);
    return t != t ? (uint16_t)0 : (uint16_t)((int)r * 257);
}

__global__ __launch_bounds__(kClassThreads) void class_paint_kernel(const double* __restrict__ classes,
                                                                   const int64_t* __restrict__ offsets, int64_t total, int B,
                                                                   const uint32_t* __restrict__ present,
                                                                   const uint64_t* __restrict__ table, int T,
                                                                   uint64_t* __restrict__ colors, uint16_t* __restrict__ rgb,
                                                                   unsigned long long* __restrict__ short_table) {
    __shared__ uint32_t s_bits[kClassWords];
    __shared__ int s_pre[kClassWords];
    __shared__ int s_wave[kClassThreads / 64];
    const int t = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * kClassChunk;
    sn::for_tiles(offsets, B, base, kClassChunk, total, [&](int b, int64_t, int64_t, int64_t from, int64_t to) {
        __syncthreads();   // the previous tile's tables have been read
        {
            uint32_t w[kClassItems];
            int pre[kClassItems];
            words_and_prefix(present + (size_t)b * kClassWords, w, pre, s_wave);
#pragma unroll
            for (int q = 0; q < kClassItems; ++q) {
                s_bits[t * kClassItems + q] = w[q];
                s_pre[t * kClassItems + q] = pre[q];
            }
        }
        __syncthreads();
        int nshort = 0;
        const int first = (int)((from - base) / kClassThreads), last = (int)((to - 1 - base) / kClassThreads);
        for (int k0 = first; k0 <= last; k0 += kClassBatch) {
            double v[kClassBatch];
            bool in[kClassBatch];
#pragma unroll
            for (int q = 0; q < kClassBatch; ++q) {
                const int64_t i = base + (int64_t)(k0 + q) * kClassThreads + t;   // (rounds behind `last` are at or behind `to`)
                in[q] = i >= from && i < to;
                v[q] = in[q] ? classes[i] : 0.0;
            }
#pragma unroll
            for (int q = 0; q < kClassBatch; ++q) {
                if (!in[q]) continue;
                const int64_t i = base + (int64_t)(k0 + q) * kClassThreads + t;
                const int c = class_of(v[q]);
                int rank = -1;
                if (c >= 0) rank = s_pre[c >> 5] + __popc(s_bits[c >> 5] & ((1u << (c & 31)) - 1u));
                const bool isshort = rank >= T;
                const bool ok = c >= 0 && !isshort;
                uint64_t v0 = kNanBits, v1 = kNanBits, v2 = kNanBits;
                if (ok) {
                    const uint64_t* row = table + (size_t)rank * 3;
                    v0 = row[0];
                    v1 = row[1];
                    v2 = row[2];
                }
                if (colors) {
                    uint64_t* o = colors + i * 3;
                    o[0] = v0;
                    o[1] = v1;
                    o[2] = v2;
                }
                if (rgb) {
                    uint16_t* o = rgb + i * 3;
                    o[0] = ok ? rgb16_of(__longlong_as_double((long long)v0)) : (uint16_t)0;
                    o[1] = ok ? rgb16_of(__longlong_as_double((long long)v1)) : (uint16_t)0;
                    o[2] = ok ? rgb16_of(__longlong_as_double((long long)v2)) : (uint16_t)0;
                }
                nshort += isshort;
            }
        }
        nshort = sn::wave_reduce(nshort, [](int a, int b) { return a + b; });
        if ((t & 63) == 0 && nshort)
            __hip_atomic_fetch_add(short_table + b, (unsigned long long)nshort, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    });
}

bool shape_served(int64_t total, int B) { return total > 0 && B > 0 && total <= kMaxTotal && B <= kMaxB; }

// what the three entries ask of their batch; `rows` names the packed array in the error text
int check_batch(const char* what, const char* rows, const void* data, const int64_t* offsets, int64_t total, int B) {
    if (!data) return sn::fail(SN_ERR_INVALID_ARG, "%s: %s is null", what, rows);
    if (!offsets) return sn::fail(SN_ERR_INVALID_ARG, "%s: offsets is null", what);
    if (total <= 0) return sn::fail(SN_ERR_INVALID_ARG, "%s: total must be positive (got %lld)", what, (long long)total);
    if (B <= 0) return sn::fail(SN_ERR_INVALID_ARG, "%s: B must be positive (got %d)", what, B);
    if (!shape_served(total, B))
        return sn::fail(SN_ERR_UNSUPPORTED, "%s: total=%lld, B=%d beyond what is served (total <= 2^33, B <= %d)", what,
                        (long long)total, B, kMaxB);
    return SN_OK;
}

}  // namespace

extern "C" int sn_voxel_classes_chunk_points(void) { return kWaveChunk; }
extern "C" int sn_class_chunk_points(void) { return kClassChunk; }

extern "C" int sn_voxel_classes(const double* pts, const double* labels, const int64_t* offsets, int64_t total, int B,
                                const double* desc, int nx, int ny, int nz, int flags, double* grid, int64_t* unbinned,
                                int64_t* nan_labels, sn_stream_t stream) {
    const char* what = "sn_voxel_classes";
    const int rc = check_batch(what, "pts", pts, offsets, total, B);
    if (rc != SN_OK) return rc;
    if (!labels) return sn::fail(SN_ERR_INVALID_ARG, "%s: labels is null", what);
    if (!desc) return sn::fail(SN_ERR_INVALID_ARG, "%s: desc is null", what);
    if (!grid) return sn::fail(SN_ERR_INVALID_ARG, "%s: grid is null", what);
    if (!unbinned) return sn::fail(SN_ERR_INVALID_ARG, "%s: unbinned is null", what);
    if (!nan_labels) return sn::fail(SN_ERR_INVALID_ARG, "%s: nan_labels is null", what);
    if (nx <= 0 || ny <= 0 || nz <= 0)
        return sn::fail(SN_ERR_INVALID_ARG, "%s: non-positive grid extent (%d, %d, %d)", what, nx, ny, nz);
    if (flags & ~SN_VOXEL_CLASSES_NO_SKIP) return sn::fail(SN_ERR_INVALID_ARG, "%s: unknown flags %d", what, flags);
    const size_t lds = ((size_t)nx + (size_t)ny + (size_t)nz + 3) * sizeof(double);
    if (lds > 64 * 1024) return sn::fail(SN_ERR_UNSUPPORTED, "%s: edge tables beyond 64 KiB of LDS", what);
    const int64_t V = (int64_t)nx * ny * nz;
    if (V >= ((int64_t)1 << 31)) return sn::fail(SN_ERR_UNSUPPORTED, "%s: nx * ny * nz >= 2^31", what);
    if ((uintptr_t)pts % 8 || (uintptr_t)labels % 8 || (uintptr_t)offsets % 8 || (uintptr_t)desc % 8 || (uintptr_t)grid % 8 ||
        (uintptr_t)unbinned % 8 || (uintptr_t)nan_labels % 8)
        return sn::fail(SN_ERR_INVALID_ARG, "%s: pts / labels / offsets / desc / grid / unbinned / nan_labels must be 8-byte aligned",
                        what);
    hipStream_t s = sn::as_stream(stream);
    const int64_t cells = (int64_t)B * V;
    const int64_t nchunks = (total + kWaveChunk - 1) / kWaveChunk;
    unsigned long long* g = reinterpret_cast<unsigned long long*>(grid);
    unsigned long long* u = reinterpret_cast<unsigned long long*>(unbinned);
    unsigned long long* n = reinterpret_cast<unsigned long long*>(nan_labels);
    zero(g, cells, u, n, B, s);
    const dim3 blocks((unsigned)nchunks), threads(kWaveLanes);
    if (flags & SN_VOXEL_CLASSES_NO_SKIP)
        hipLaunchKernelGGL(classes_points_kernel<false>, blocks, threads, lds, s, pts, labels, offsets, total, B, desc, nx, ny, nz,
                           g, u, n);
    else
        hipLaunchKernelGGL(classes_points_kernel<true>, blocks, threads, lds, s, pts, labels, offsets, total, B, desc, nx, ny, nz,
                           g, u, n);
    const int64_t want = (cells + 256 * 4 - 1) / (256 * 4);
    hipLaunchKernelGGL(classes_decode_kernel, dim3((unsigned)(want < 8192 ? want : 8192)), dim3(256), 0, s, g, cells);
    return sn::check_launch(what);
}

extern "C" int sn_class_census(const double* classes, const int64_t* offsets, int64_t total, int B, uint32_t* present,
                               int64_t* bad, sn_stream_t stream) {
    const char* what = "sn_class_census";
    const int rc = check_batch(what, "classes", classes, offsets, total, B);
    if (rc != SN_OK) return rc;
    if (!present) return sn::fail(SN_ERR_INVALID_ARG, "%s: present is null", what);
    if (!bad) return sn::fail(SN_ERR_INVALID_ARG, "%s: bad is null", what);
    if ((uintptr_t)classes % 8 || (uintptr_t)offsets % 8 || (uintptr_t)bad % 8 || (uintptr_t)present % 4)
        return sn::fail(SN_ERR_INVALID_ARG, "%s: classes / offsets / bad must be 8-byte, present 4-byte aligned", what);
    hipStream_t s = sn::as_stream(stream);
    zero(present, (int64_t)B * kClassWords, reinterpret_cast<unsigned long long*>(bad), (unsigned long long*)nullptr, B, s);
    const int64_t nchunks = (total + kClassChunk - 1) / kClassChunk;
    hipLaunchKernelGGL(class_census_kernel, dim3((unsigned)nchunks), dim3(kClassThreads), 0, s, classes, offsets, total, B, present,
                       reinterpret_cast<unsigned long long*>(bad));
    return sn::check_launch(what);
}

extern "C" int sn_class_paint(const double* classes, const int64_t* offsets, int64_t total, int B, const uint32_t* present,
                              const double* table, int T, double* colors, uint16_t* rgb, double* unique, int U_max,
                              int64_t* n_unique, int64_t* short_table, sn_stream_t stream) {
    const char* what = "sn_class_paint";
    const int rc = check_batch(what, "classes", classes, offsets, total, B);
    if (rc != SN_OK) return rc;
    if (!present) return sn::fail(SN_ERR_INVALID_ARG, "%s: present is null", what);
    if (!table) return sn::fail(SN_ERR_INVALID_ARG, "%s: table is null", what);
    if (!n_unique) return sn::fail(SN_ERR_INVALID_ARG, "%s: n_unique is null", what);
    if (!short_table) return sn::fail(SN_ERR_INVALID_ARG, "%s: short_table is null", what);
    if (!colors && !rgb) return sn::fail(SN_ERR_INVALID_ARG, "%s: neither colors nor rgb is given", what);
    if (T <= 0) return sn::fail(SN_ERR_INVALID_ARG, "%s: T must be positive (got %d)", what, T);
    if (unique && U_max <= 0) return sn::fail(SN_ERR_INVALID_ARG, "%s: U_max must be positive with unique (got %d)", what, U_max);
    if ((uintptr_t)classes % 8 || (uintptr_t)offsets % 8 || (uintptr_t)table % 8 || (uintptr_t)colors % 8 ||
        (uintptr_t)unique % 8 || (uintptr_t)n_unique % 8 || (uintptr_t)short_table % 8 || (uintptr_t)present % 4 ||
        (uintptr_t)rgb % 2)
        return sn::fail(SN_ERR_INVALID_ARG,
                        "%s: classes / offsets / table / colors / unique / n_unique / short_table must be 8-byte, present 4-byte, "
                        "rgb 2-byte aligned", what);
    hipStream_t s = sn::as_stream(stream);
    hipLaunchKernelGGL(class_unique_kernel, dim3((unsigned)B), dim3(kClassThreads), 0, s, present, unique, U_max, n_unique,
                       short_table);
    const int64_t nchunks = (total + kClassChunk - 1) / kClassChunk;
    hipLaunchKernelGGL(class_paint_kernel, dim3((unsigned)nchunks), dim3(kClassThreads), 0, s, classes, offsets, total, B, present,
                       reinterpret_cast<const uint64_t*>(table), T, reinterpret_cast<uint64_t*>(colors), rgb,
                       reinterpret_cast<unsigned long long*>(short_table));
    return sn::check_launch(what);
}
