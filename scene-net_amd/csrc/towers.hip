// K8 -- tower proposals: DBSCAN over the voxels of a thresholded prediction (sn_tower_proposals).
// replaces: eda.extract_towers (utils/pcd_processing.py:577-651: open3d cluster_dbscan + a pandas group-by per tile on
// the host) behind prob_to_label (utils/voxelization.py:304-323), as utils/observer_utils.py:397-473, 556- call it.
//
// On a lattice DBSCAN needs no tree: a voxel's eps-neighbourhood is a fixed stencil of offsets, and every (d0, d1) row
// of that stencil is an interval of 2 * hw + 1 voxels along axis 2.  With one bit per voxel (rows padded to whole 64-bit
// words) an interval is one or two masked words: neighbour counts are population counts, and the neighbours themselves
// are the set bits.  Six launches, tiles independent throughout:
//   1 threshold  grid >= tau -> "positive" bitmap (a wave per word, one ballot)
//   2 core       positive and >= min_points positives inside the stencil -> "core" bitmap; parent[v] = v for cores
//   3 union      lock-free union-find over the cores (union_find.h): every core unites with the cores of the backward
//                half of its stencil; a component's root is its smallest index
//   4 flatten    parent[v] = root(v) (read-only walks: only v's own thread writes parent[v]) and the "root" bitmap
//   5 rank       per tile, the exclusive prefix of the root bitmap's population counts: cluster id = number of roots in
//                front of a root = rank by smallest core voxel; n_towers; the tile's statistics rows initialised
//   6 finish     labels (cores: their root's rank; borders: the smallest root among the cores in their stencil) and the
//                integer statistics, summed per wave first and then added with 64-bit integer atomics
// Launches 2, 3 and 6 read a tile's bitmap many times: it is staged in LDS where it fits (64^3: 32 KiB) and read from the
// workspace (L2) where it does not (128^3: 256 KiB); the two forms are the same code behind one accessor.
// Every output is an integer function of the input; all accumulation is integer: results do not depend on scheduling.
//
// Bound: launches 1 and 6 by HBM (the grid read once, the labels written once); 2, 3 by LDS / L2 reads per positive voxel.
#include "common.h"
#include "scan.h"
#include "union_find.h"
#include <cmath>
#include <type_traits>

namespace {

constexpr int kMaxRadius = 10;                                       // voxels per axis
constexpr int kMaxRows = (2 * kMaxRadius + 1) * (2 * kMaxRadius + 1);
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kChunkWords = 256;             // bitmap words one workgroup of launches 2, 3, 6 works through
constexpr int kLdsBytes = 64 * 1024;         // a tile's bitmap is staged in LDS up to this size
constexpr int kRankThreads = 1024;
constexpr int64_t kMaxTileWords = (int64_t)1 << 18;    // 2^24 padded voxels per tile (256^3)
constexpr int64_t kMaxWords = (int64_t)1 << 30;
constexpr int kMaxTiles = 65535;                      // the tile index is gridDim.y of launches 2, 3 and 6
constexpr long long kMinInit = (long long)1 << 62;

using bf16 = __bf16;

// one stencil row in 32 bits: (d0 + kMaxRadius) | (d1 + kMaxRadius) << 8 | hw << 16; rows ascend in (d0, d1)
struct Stencil {
    int nrows;
    uint32_t row[kMaxRows];
};

struct Shape {
    int B, n0, n1, n2;
    int W;     // words per (i0, i1) row
    int N;     // words per tile = n0 * n1 * W
};

__device__ __forceinline__ uint64_t bits_between(int a, int b) {   // bits a..b of a word, 0 <= a <= b <= 63
    return (~0ull << a) & (~0ull >> (63 - b));
}

// the tile's bitmap: LDS copy or the workspace itself
template <bool kLds>
struct Bitmap {
    const uint64_t* p;
    __device__ __forceinline__ uint64_t operator[](int i) const { return p[i]; }
};

template <bool kLds>
__device__ __forceinline__ Bitmap<kLds> stage_bitmap(const uint64_t* tile_words, int N, uint64_t* lds) {
    if constexpr (kLds) {
        for (int i = threadIdx.x; i < N; i += kThreads) lds[i] = tile_words[i];
        __syncthreads();
        return Bitmap<kLds>{lds};
    } else {
        return Bitmap<kLds>{tile_words};
    }
}

// The words of stencil row `r` around voxel (i0, i1, i2), clipped at the grid faces: m0 sits in word `at`, m1 in word
// at + 1 (an interval of at most 2 * kMaxRadius + 1 = 21 bits touches two words at most).  false: the row lies outside.
template <bool kLds>
__device__ __forceinline__ bool stencil_row(const Bitmap<kLds>& bm, const Shape& sh, uint32_t r, int i0, int i1, int i2,
                                            int& at, uint64_t& m0, uint64_t& m1) {
    const int j0 = i0 + (int)(r & 0xffu) - kMaxRadius, j1 = i1 + (int)((r >> 8) & 0xffu) - kMaxRadius;
    if ((unsigned)j0 >= (unsigned)sh.n0 || (unsigned)j1 >= (unsigned)sh.n1) return false;
    const int hw = (int)(r >> 16);
    const int lo = i2 - hw < 0 ? 0 : i2 - hw, hi = i2 + hw > sh.n2 - 1 ? sh.n2 - 1 : i2 + hw;
    const int wl = lo >> 6, wh = hi >> 6;
    at = (j0 * sh.n1 + j1) * sh.W + wl;
    if (wl == wh) {
        m0 = bm[at] & bits_between(lo & 63, hi & 63);
        m1 = 0;
    } else {
        m0 = bm[at] & bits_between(lo & 63, 63);
        m1 = bm[at + 1] & bits_between(0, hi & 63);
    }
    return true;
}

template <typename T> struct Wide { using type = T; };
template <> struct Wide<bf16> { using type = float; };

// ---- 1: positive bitmap.  A wave per word: lane = bit.  Padding bits (i2 >= n2) stay 0.
template <typename T>
__global__ __launch_bounds__(kThreads) void towers_threshold_kernel(const T* __restrict__ grid, Shape sh,
                                                                    typename Wide<T>::type tau,
                                                                    uint64_t* __restrict__ pos) {
    using C = typename Wide<T>::type;
    const int lane = threadIdx.x & 63;
    const int64_t total = (int64_t)sh.B * sh.N;
    const int64_t stride = (int64_t)gridDim.x * kWaves;
    for (int64_t w = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6); w < total; w += stride) {
        const int64_t row = w / sh.W;                 // (b * n0 + i0) * n1 + i1
        const int i2 = (int)(w - row * sh.W) * 64 + lane;
        bool p = false;
        if (i2 < sh.n2) {
            const T v = grid[row * sh.n2 + i2];
            if constexpr (std::is_same<T, uint8_t>::value) p = v != 0;
            else p = (C)v >= tau;                     // NaN compares false
        }
        const uint64_t m = __ballot(p);
        if (lane == 0) pos[w] = m;
    }
}

// ---- 2: core bitmap and the cores' parent[v] = v
template <bool kLds>
__global__ __launch_bounds__(kThreads) void towers_core_kernel(const uint64_t* __restrict__ pos, Shape sh, Stencil st,
                                                               int min_points, uint64_t* __restrict__ core,
                                                               int32_t* __restrict__ parent) {
    extern __shared__ uint64_t lds[];
    const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t* tile = pos + (size_t)b * sh.N;
    const Bitmap<kLds> bm = stage_bitmap<kLds>(tile, sh.N, lds);
    const int w_end = min((int)(blockIdx.x + 1) * kChunkWords, sh.N);
    for (int w = blockIdx.x * kChunkWords + wave; w < w_end; w += kWaves) {
        const uint64_t pw = bm[w];
        bool is_core = false;
        if ((pw >> lane) & 1ull) {
            const int row = w / sh.W, i0 = row / sh.n1, i1 = row - i0 * sh.n1, i2 = (w - row * sh.W) * 64 + lane;
            int cnt = 0;
            for (int k = 0; k < st.nrows && cnt < min_points; ++k) {
                int at;
                uint64_t m0, m1;
                if (stencil_row(bm, sh, st.row[k], i0, i1, i2, at, m0, m1)) cnt += __popcll(m0) + __popcll(m1);
            }
            is_core = cnt >= min_points;
        }
        const uint64_t cw = __ballot(is_core);
        if (lane == 0) core[(size_t)b * sh.N + w] = cw;
        if (is_core) parent[((size_t)b * sh.N + w) * 64 + lane] = w * 64 + lane;
    }
}

// ---- union-find over parent[] (union_find.h): the indices are tile-local padded voxel indices

// ---- 3: every core unites with the cores of the backward half of its stencil (the forward half is the other voxel's
// backward half).  In its own row the nearest core in front suffices: the cores between are that one's business.
template <bool kLds>
__global__ __launch_bounds__(kThreads) void towers_union_kernel(const uint64_t* __restrict__ core, Shape sh, Stencil st,
                                                                int32_t* __restrict__ parent) {
    extern __shared__ uint64_t lds[];
    const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const Bitmap<kLds> bm = stage_bitmap<kLds>(core + (size_t)b * sh.N, sh.N, lds);
    int32_t* par = parent + (size_t)b * sh.N * 64;
    const int w_end = min((int)(blockIdx.x + 1) * kChunkWords, sh.N);
    const uint32_t centre = (uint32_t)kMaxRadius | ((uint32_t)kMaxRadius << 8);
    for (int w = blockIdx.x * kChunkWords + wave; w < w_end; w += kWaves) {
        const uint64_t cw = bm[w];
        if (!((cw >> lane) & 1ull)) continue;
        const int row = w / sh.W, i0 = row / sh.n1, i1 = row - i0 * sh.n1, i2 = (w - row * sh.W) * 64 + lane;
        int32_t root = w * 64 + lane;
        for (int k = 0; k < st.nrows; ++k) {
            const uint32_t r = st.row[k];
            const bool own_row = (r & 0xffffu) == centre;
            int at;
            uint64_t m0, m1;
            if (!stencil_row(bm, sh, r, i0, i1, i2, at, m0, m1)) continue;
            if (own_row) {
                // the bits in front of this voxel; the interval starts in word `at`, this voxel sits in word w
                if (at == w) m0 &= ~(~0ull << lane), m1 = 0;
                else m1 &= ~(~0ull << lane);
                if (m1) root = uf_unite(par, root, (at + 1) * 64 + 63 - __clzll(m1));
                else if (m0) root = uf_unite(par, root, at * 64 + 63 - __clzll(m0));
                break;   // rows ascend in (d0, d1): what follows is the forward half
            }
            while (m0) {
                root = uf_unite(par, root, at * 64 + __ffsll((unsigned long long)m0) - 1);
                m0 &= m0 - 1;
            }
            while (m1) {
                root = uf_unite(par, root, (at + 1) * 64 + __ffsll((unsigned long long)m1) - 1);
                m1 &= m1 - 1;
            }
        }
    }
}

// ---- 4: parent[v] = root(v) for every core, and the root bitmap.  No hooks happen in this launch, so roots stay roots;
// parent[v] is written by v's own thread only, and a reader sees the old ancestor or the root.
__global__ __launch_bounds__(kThreads) void towers_flatten_kernel(const uint64_t* __restrict__ core, Shape sh,
                                                                  int32_t* __restrict__ parent,
                                                                  uint64_t* __restrict__ rootbits) {
    const int lane = threadIdx.x & 63;
    const int64_t total = (int64_t)sh.B * sh.N;
    const int64_t stride = (int64_t)gridDim.x * kWaves;
    for (int64_t w = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6); w < total; w += stride) {
        const uint64_t cw = core[w];
        bool is_root = false;
        if ((cw >> lane) & 1ull) {
            const int64_t b = w / sh.N;
            const int32_t v = (int32_t)(w - b * sh.N) * 64 + lane;
            int32_t* par = parent + b * sh.N * 64;
            const int32_t r = uf_find_readonly(par, v);
            if (r != v) uf_store(par + v, r);
            is_root = r == v;
        }
        const uint64_t m = __ballot(is_root);
        if (lane == 0) rootbits[w] = m;
    }
}

// ---- 5: one workgroup per tile.  prefix[w] = roots in the words before w; n_towers; the tile's statistics rows:
// zero, the minima of present clusters at kMinInit, first_core_index set here.
__global__ __launch_bounds__(kRankThreads) void towers_rank_kernel(const uint64_t* __restrict__ rootbits, Shape sh,
                                                                   int max_towers, int32_t* __restrict__ prefix,
                                                                   int32_t* __restrict__ n_towers,
                                                                   long long* __restrict__ stats) {
    __shared__ int32_t wave_sum[kRankThreads / 64];
    const int b = blockIdx.x, tid = threadIdx.x;
    const uint64_t* bits = rootbits + (size_t)b * sh.N;
    int32_t* pre = prefix + (size_t)b * sh.N;
    const int per = (sh.N + kRankThreads - 1) / kRankThreads;   // a contiguous run of words per thread
    const int w0 = min(tid * per, sh.N), w1 = min(w0 + per, sh.N);
    int32_t mine = 0;
    for (int w = w0; w < w1; ++w) mine += __popcll(bits[w]);
    int32_t before[1] = {mine};
    const int32_t total = sn::block_exclusive<kRankThreads, 1>(before, wave_sum);
    int32_t run = before[0];                                      // roots in the words of the threads in front
    const int K = total < max_towers ? total : max_towers;
    long long* rows = stats + (size_t)b * max_towers * SN_TOWER_NSTAT;
    for (int i = tid; i < max_towers * SN_TOWER_NSTAT; i += kRankThreads) {
        const int id = i / SN_TOWER_NSTAT, col = i - id * SN_TOWER_NSTAT;
        if (col != SN_TOWER_NSTAT - 1 || id >= K) rows[i] = (id < K && col >= 5 && col <= 7) ? kMinInit : 0;
    }
    for (int w = w0; w < w1; ++w) {
        pre[w] = run;
        uint64_t m = bits[w];
        while (m && run < max_towers) {   // first_core_index: the root's index in memory order (rows unpadded)
            const int bit = __ffsll((unsigned long long)m) - 1;
            const int row = w / sh.W;
            rows[(size_t)run * SN_TOWER_NSTAT + SN_TOWER_NSTAT - 1] = (long long)row * sh.n2 + (w - row * sh.W) * 64 + bit;
            ++run;
            m &= m - 1;
        }
        run += __popcll(m);
    }
    if (tid == 0) n_towers[b] = total;
}

// ---- 6: labels and statistics
template <bool kLds>
__global__ __launch_bounds__(kThreads) void towers_finish_kernel(const uint64_t* __restrict__ pos,
                                                                 const uint64_t* __restrict__ core,
                                                                 const uint64_t* __restrict__ rootbits,
                                                                 const int32_t* __restrict__ prefix,
                                                                 const int32_t* __restrict__ parent, Shape sh, Stencil st,
                                                                 int max_towers, int32_t* __restrict__ labels,
                                                                 long long* __restrict__ stats) {
    extern __shared__ uint64_t lds[];
    const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t tile = (size_t)b * sh.N;
    const Bitmap<kLds> bm = stage_bitmap<kLds>(core + tile, sh.N, lds);
    const int32_t* par = parent + tile * 64;
    unsigned long long* rows = reinterpret_cast<unsigned long long*>(stats) + (size_t)b * max_towers * SN_TOWER_NSTAT;
    const int w_end = min((int)(blockIdx.x + 1) * kChunkWords, sh.N);
    for (int w = blockIdx.x * kChunkWords + wave; w < w_end; w += kWaves) {
        const uint64_t pw = pos[tile + w], cw = bm[w];
        const int row = w / sh.W, i0 = row / sh.n1, i1 = row - i0 * sh.n1, i2 = (w - row * sh.W) * 64 + lane;
        int32_t id = -1;
        if (pw) {   // (wave-uniform)
            int32_t root = -1;
            if ((cw >> lane) & 1ull) {
                root = par[w * 64 + lane];
            } else if ((pw >> lane) & 1ull) {
                // border: the smallest root among the cores of the stencil = the smallest cluster id
                int32_t best = 0x7fffffff;
                for (int k = 0; k < st.nrows; ++k) {
                    int at;
                    uint64_t m0, m1;
                    if (!stencil_row(bm, sh, st.row[k], i0, i1, i2, at, m0, m1)) continue;
                    while (m0) {
                        best = min(best, par[at * 64 + __ffsll((unsigned long long)m0) - 1]);
                        m0 &= m0 - 1;
                    }
                    while (m1) {
                        best = min(best, par[(at + 1) * 64 + __ffsll((unsigned long long)m1) - 1]);
                        m1 &= m1 - 1;
                    }
                }
                if (best != 0x7fffffff) root = best;
            }
            if (root >= 0) {
                const int rw = root >> 6, rb = root & 63;
                id = prefix[tile + rw] + __popcll(rootbits[tile + rw] & ~(~0ull << rb));
            }
        }
        if (i2 < sh.n2) labels[((size_t)b * sh.n0 * sh.n1 + row) * sh.n2 + i2] = id;
        // statistics: the lanes of one cluster are summed in the wave (they share i0 and i1), one lane adds
        const bool has = id >= 0 && id < max_towers;
        uint64_t todo = __ballot(has);
        while (todo) {
            const int leader = __ffsll((unsigned long long)todo) - 1;
            const int32_t lid = __shfl(id, leader, 64);
            const bool mine = has && id == lid;
            const uint64_t m = __ballot(mine);
            todo &= ~m;
            const long long s2 = sn::wave_reduce(mine ? (long long)i2 : 0ll, [](long long a, long long b) { return a + b; });
            if (lane == leader) {
                const unsigned long long cnt = __popcll(m);
                const int base2 = i2 - lane;
                unsigned long long* r = rows + (size_t)lid * SN_TOWER_NSTAT;
                atomicAdd(r + 0, cnt);
                atomicAdd(r + 1, (unsigned long long)__popcll(m & cw));
                atomicAdd(r + 2, cnt * (unsigned long long)i0);
                atomicAdd(r + 3, cnt * (unsigned long long)i1);
                atomicAdd(r + 4, (unsigned long long)s2);
                atomicMin(r + 5, (unsigned long long)i0);
                atomicMin(r + 6, (unsigned long long)i1);
                atomicMin(r + 7, (unsigned long long)(base2 + __ffsll((unsigned long long)m) - 1));
                atomicMax(r + 8, (unsigned long long)i0);
                atomicMax(r + 9, (unsigned long long)i1);
                atomicMax(r + 10, (unsigned long long)(base2 + 63 - __clzll(m)));
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------ host
// (d0 s0)^2 + (d1 s1)^2 + (d2 s2)^2 <= eps^2 in fp64, in exactly this form (built with -ffp-contract=off)
bool inside(double eps, const double* s, int d0, int d1, int d2) {
    const double a = d0 * s[0], b = d1 * s[1], c = d2 * s[2];
    return a * a + b * b + c * c <= eps * eps;
}

// SN_OK and the packed rows, or the error code (message set)
int build_stencil(const char* who, double eps, const double* voxel_size_host, Stencil& st, int64_t* n_offsets) {
    if (!(eps > 0.0) || !std::isfinite(eps)) return sn::fail(SN_ERR_INVALID_ARG, "%s: eps must be positive and finite", who);
    double s[3] = {1.0, 1.0, 1.0};
    if (voxel_size_host)
        for (int k = 0; k < 3; ++k) {
            s[k] = voxel_size_host[k];
            if (!(s[k] > 0.0) || !std::isfinite(s[k]))
                return sn::fail(SN_ERR_INVALID_ARG, "%s: voxel_size must be positive and finite", who);
        }
    const int over = kMaxRadius + 1;
    if (inside(eps, s, over, 0, 0) || inside(eps, s, 0, over, 0) || inside(eps, s, 0, 0, over))
        return sn::fail(SN_ERR_UNSUPPORTED, "%s: eps reaches more than %d voxels along an axis", who, kMaxRadius);
    st.nrows = 0;
    int64_t n = 0;
    for (int d0 = -kMaxRadius; d0 <= kMaxRadius; ++d0)
        for (int d1 = -kMaxRadius; d1 <= kMaxRadius; ++d1) {
            if (!inside(eps, s, d0, d1, 0)) continue;
            int hw = 0;
            while (hw < kMaxRadius && inside(eps, s, d0, d1, hw + 1)) ++hw;
            st.row[st.nrows++] = (uint32_t)(d0 + kMaxRadius) | ((uint32_t)(d1 + kMaxRadius) << 8) | ((uint32_t)hw << 16);
            n += 2 * hw + 1;
        }
    if (n_offsets) *n_offsets = n;
    return SN_OK;
}

bool shape_of(int B, int n0, int n1, int n2, Shape& sh) {
    if (B <= 0 || n0 <= 0 || n1 <= 0 || n2 <= 0) return false;
    const int64_t W = ((int64_t)n2 + 63) / 64;
    const int64_t N = (int64_t)n0 * n1 * W;
    if (N > kMaxTileWords || N * B > kMaxWords || B > kMaxTiles) return false;
    sh = Shape{B, n0, n1, n2, (int)W, (int)N};
    return true;
}

size_t ws_bytes_of(const Shape& sh) {
    // positive, core and root bitmaps (u64), the root prefix (i32), parent (i32 per padded voxel)
    return ((size_t)sh.B * sh.N * (3 * 8 + 4 + 64 * 4) + 7) / 8 * 8;   // (a whole number of 8-byte words)
}

float round_bf16(double tau) {   // to fp32, then to nearest even: how torch rounds a Python scalar for a bf16 comparison
    const float f = (float)tau;
    uint32_t u;
    __builtin_memcpy(&u, &f, 4);
    u = (u + 0x7fffu + ((u >> 16) & 1u)) & 0xffff0000u;
    float r;
    __builtin_memcpy(&r, &u, 4);
    return r;
}

int stream_blocks(int64_t words) {   // launches 1 and 4: a wave per word, grid-strided beyond 4096 workgroups
    const int64_t want = (words + kWaves - 1) / kWaves;
    return (int)(want < 4096 ? want : 4096);
}

int run(const void* grid, int dtype, int B, int n0, int n1, int n2, double tau, double eps, const double* voxel_size_host,
        int min_points, int max_towers, void* ws, size_t ws_bytes, int32_t* labels, int32_t* n_towers, int64_t* stats,
        int first, int last, sn_stream_t stream) {
    const char* who = "sn_tower_proposals";
    if (!grid || !ws || !labels || !n_towers) return sn::fail(SN_ERR_INVALID_ARG, "%s: null pointer", who);
    if (B <= 0 || n0 <= 0 || n1 <= 0 || n2 <= 0) return sn::fail(SN_ERR_INVALID_ARG, "%s: B and the extents must be positive", who);
    if (min_points < 1) return sn::fail(SN_ERR_INVALID_ARG, "%s: min_points must be at least 1", who);
    if (max_towers < 0 || (max_towers > 0 && !stats))
        return sn::fail(SN_ERR_INVALID_ARG, "%s: max_towers must not be negative, and stats is needed unless it is 0", who);
    size_t esz = 0;
    switch (dtype) {
        case SN_F32: esz = 4; break;
        case SN_BF16: esz = 2; break;
        case SN_F64: esz = 8; break;
        case SN_U8:
        case SN_OCC8: esz = 1; break;
        default:
            return sn::fail(dtype == SN_I32 ? SN_ERR_UNSUPPORTED : SN_ERR_INVALID_ARG,
                            "%s: grid dtype %d not accepted (SN_F32 | SN_BF16 | SN_F64 | SN_U8 | SN_OCC8)", who, dtype);
    }
    if (esz > 1 && !(tau > 0.0 && tau < 1.0)) return sn::fail(SN_ERR_INVALID_ARG, "%s: tau must lie in (0, 1)", who);
    Stencil st;
    if (int e = build_stencil(who, eps, voxel_size_host, st, nullptr)) return e;
    Shape sh;
    if (!shape_of(B, n0, n1, n2, sh))
        return sn::fail(SN_ERR_UNSUPPORTED, "%s: at most 2^24 voxels per tile (rows padded to 64), 2^36 per call and 65535 tiles", who);
    if ((int64_t)max_towers * SN_TOWER_NSTAT > (int64_t)1 << 30)
        return sn::fail(SN_ERR_UNSUPPORTED, "%s: max_towers too large", who);
    if ((uintptr_t)grid % esz || (uintptr_t)ws % 8 || (uintptr_t)labels % 4 || (uintptr_t)n_towers % 4 || (uintptr_t)stats % 8)
        return sn::fail(SN_ERR_INVALID_ARG, "%s: grid must be aligned to its element, ws / stats to 8 bytes, labels / "
                        "n_towers to 4", who);
    const size_t need = ws_bytes_of(sh);
    if (ws_bytes < need)
        return sn::fail(SN_ERR_INVALID_ARG, "%s: ws holds %zu bytes, %zu needed (sn_towers_ws_bytes)", who, ws_bytes, need);

    hipStream_t s = sn::as_stream(stream);
    const size_t words = (size_t)B * sh.N;
    uint64_t* pos = static_cast<uint64_t*>(ws);
    uint64_t* core = pos + words;
    uint64_t* rootbits = core + words;
    int32_t* parent = reinterpret_cast<int32_t*>(rootbits + words);
    int32_t* prefix = parent + words * 64;
    long long* st64 = reinterpret_cast<long long*>(stats);
    const bool in_lds = (size_t)sh.N * 8 <= (size_t)kLdsBytes;
    const size_t lds = in_lds ? (size_t)sh.N * 8 : 0;
    const dim3 tiles((unsigned)((sh.N + kChunkWords - 1) / kChunkWords), (unsigned)B), block(kThreads);
    const dim3 flat((unsigned)stream_blocks((int64_t)words));

    if (first <= 1 && last >= 1) {
        switch (dtype) {
            case SN_F32:
                hipLaunchKernelGGL(towers_threshold_kernel<float>, flat, block, 0, s, (const float*)grid, sh, (float)tau, pos);
                break;
            case SN_BF16:
                hipLaunchKernelGGL(towers_threshold_kernel<bf16>, flat, block, 0, s, (const bf16*)grid, sh, round_bf16(tau),
                                   pos);
                break;
            case SN_F64:
                hipLaunchKernelGGL(towers_threshold_kernel<double>, flat, block, 0, s, (const double*)grid, sh, tau, pos);
                break;
            default:
                hipLaunchKernelGGL(towers_threshold_kernel<uint8_t>, flat, block, 0, s, (const uint8_t*)grid, sh, (uint8_t)0,
                                   pos);
                break;
        }
        if (int e = sn::check_launch("sn_tower_proposals(threshold)")) return e;
    }
    if (first <= 2 && last >= 2) {
        if (in_lds) hipLaunchKernelGGL(towers_core_kernel<true>, tiles, block, lds, s, pos, sh, st, min_points, core, parent);
        else hipLaunchKernelGGL(towers_core_kernel<false>, tiles, block, 0, s, pos, sh, st, min_points, core, parent);
        if (int e = sn::check_launch("sn_tower_proposals(core)")) return e;
    }
    if (first <= 3 && last >= 3) {
        if (in_lds) hipLaunchKernelGGL(towers_union_kernel<true>, tiles, block, lds, s, core, sh, st, parent);
        else hipLaunchKernelGGL(towers_union_kernel<false>, tiles, block, 0, s, core, sh, st, parent);
        if (int e = sn::check_launch("sn_tower_proposals(union)")) return e;
    }
    if (first <= 4 && last >= 4) {
        hipLaunchKernelGGL(towers_flatten_kernel, flat, block, 0, s, core, sh, parent, rootbits);
        if (int e = sn::check_launch("sn_tower_proposals(flatten)")) return e;
    }
    if (first <= 5 && last >= 5) {
        hipLaunchKernelGGL(towers_rank_kernel, dim3((unsigned)B), dim3(kRankThreads), 0, s, rootbits, sh, max_towers, prefix,
                           n_towers, st64);
        if (int e = sn::check_launch("sn_tower_proposals(rank)")) return e;
    }
    if (first <= 6 && last >= 6) {
        if (in_lds)
            hipLaunchKernelGGL(towers_finish_kernel<true>, tiles, block, lds, s, pos, core, rootbits, prefix, parent, sh, st,
                               max_towers, labels, st64);
        else
            hipLaunchKernelGGL(towers_finish_kernel<false>, tiles, block, 0, s, pos, core, rootbits, prefix, parent, sh, st,
                               max_towers, labels, st64);
        if (int e = sn::check_launch("sn_tower_proposals(finish)")) return e;
    }
    return SN_OK;
}

}  // namespace

extern "C" int sn_towers_stencil(double eps, const double* voxel_size_host, int32_t* rows_host, int cap,
                                 int64_t* n_offsets) {
    Stencil st;
    if (int e = build_stencil("sn_towers_stencil", eps, voxel_size_host, st, n_offsets)) return e;
    if (rows_host)
        for (int k = 0; k < st.nrows && k < cap; ++k) {
            rows_host[3 * k + 0] = (int32_t)(st.row[k] & 0xffu) - kMaxRadius;
            rows_host[3 * k + 1] = (int32_t)((st.row[k] >> 8) & 0xffu) - kMaxRadius;
            rows_host[3 * k + 2] = (int32_t)(st.row[k] >> 16);
        }
    return st.nrows;
}

extern "C" size_t sn_towers_ws_bytes(int B, int n0, int n1, int n2) {
    Shape sh;
    return shape_of(B, n0, n1, n2, sh) ? ws_bytes_of(sh) : 0;
}

extern "C" int sn_tower_proposals(const void* grid, int dtype, int B, int n0, int n1, int n2, double tau, double eps,
                                  const double* voxel_size_host, int min_points, int max_towers, void* ws, size_t ws_bytes,
                                  int32_t* labels, int32_t* n_towers, int64_t* stats, sn_stream_t stream) {
    return run(grid, dtype, B, n0, n1, n2, tau, eps, voxel_size_host, min_points, max_towers, ws, ws_bytes, labels, n_towers,
               stats, 1, SN_TOWER_LAUNCHES, stream);
}

extern "C" int sn_tower_proposals_launches(const void* grid, int dtype, int B, int n0, int n1, int n2, double tau, double eps,
                                           const double* voxel_size_host, int min_points, int max_towers, void* ws,
                                           size_t ws_bytes, int32_t* labels, int32_t* n_towers, int64_t* stats,
                                           int first, int last, sn_stream_t stream) {
    if (first < 1 || last > SN_TOWER_LAUNCHES || first > last)
        return sn::fail(SN_ERR_INVALID_ARG, "sn_tower_proposals_launches: 1 <= first <= last <= %d", SN_TOWER_LAUNCHES);
    return run(grid, dtype, B, n0, n1, n2, tau, eps, voxel_size_host, min_points, max_towers, ws, ws_bytes, labels, n_towers,
               stats, first, last, stream);
}
