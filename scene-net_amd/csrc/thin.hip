// K17 -- thinning: every point of a CSR batch is kept iff u <= thr[tile][group], the survivors compacted in scan order
// (sn_thin_count, sn_thin_scatter).
// replaces: the two downsamplers of utils/pcd_processing.py -- downsampling (:375-420) and downsampling_relative_height
//           (:423-474): a Python loop over the points that fills a dict of lists keyed by voxel_n / voxel_z, then per group
//           np.random.rand(len(group)) and `group[selected <= threshold]`.
//
// Definition (normative, include/scenenet_hip.h): point j of tile b is kept iff it is binned and u <= thr[b][g], the
// comparison taken literally (a NaN on either side keeps nothing); g is 0, K1's z index or K1's flat [z][x][y] index
// (binning.h: the text voxel.hip bins with).  u is the caller's, or Philox4x32-10 of (seed; j, tile id): a function of
// the point's place in ITS tile, never of the batch or of scheduling.
//
// Shape: K9's, its scans and ranks from scan.h -- one WAVE per workgroup, kWaveChunk = 1024 consecutive rows of the packed
// batch per workgroup, lane l holding the rows chunk * 1024 + g * 64 + l, g = 0..15.  A chunk may straddle tiles: the wave
// finds the tile of its first row by a bisection of offsets (wave-uniform, scalar loads) and walks the tiles that reach
// into the chunk (the walk of sn::for_tiles, packed_rows.h, which K18 and K24 call; written out in decide_chunk),
// one edge table in LDS at a time (one wave: the barrier around the reload costs nothing).
//   count:    the decision of every row -> ws.keep[chunk][16] (one 64-bit ballot per group), ws.unb[chunk][16] (rows that
//             no table holds), their popcounts in ws.kept[chunk] / ws.lost[chunk]; `first` by 64-bit atomic min (the z
//             rule's through nz words of LDS per wave; without groups it is one plain store per tile)
//   prefix:   two workgroups turn kept / lost into exclusive prefixes (totals in slot nchunks)
//   offsets:  thread b: rows kept in front of packed index offsets[b] = prefix of its chunk + popcount of the ballots in
//             front of it -> offsets_out[b]; the same over unb -> unbinned[b]
//   scatter:  reads the ballots (128 B per 1024 rows) instead of deciding again, ranks by mbcnt, moves 64-bit patterns.
//             With out_key and a grouped rule it decides again, with the count's own function, to find the groups
//             ([measured] deciding again where the bits would do: never faster, up to 2.3x slower with groups).
// Every slot of ws is written by exactly one workgroup; nothing waits for anything.
//
// Bound: count reads 8 B per row (u) or nothing (built-in generator, group none), 24 B more with a grouped rule and a
// gathered 8 B of thr; scatter reads 24 + 8 B and writes 24 + 8 + 8 (+ 4) B per kept row.
#include "common.h"
#include "binning.h"
#include "packed_rows.h"
#include "scan.h"

namespace {

using sn::kWaveLanes;     // scan.h: kWaveGroups groups of 64 consecutive rows held per lane, kWaveChunk rows per workgroup
using sn::kWaveGroups;
using sn::kWaveChunk;
using sn::kScanThreads;
using sn::kScanItems;
constexpr int kMaxB = 1 << 16;
constexpr int64_t kMaxTotal = (int64_t)1 << 33;

// ---- Philox4x32-10 (Salmon et al., SC'11; the constants of Random123's philox.h)
constexpr uint32_t kPhiloxM0 = 0xD2511F53u, kPhiloxM1 = 0xCD9E8D57u;
constexpr uint32_t kPhiloxW0 = 0x9E3779B9u, kPhiloxW1 = 0xBB67AE85u;

// words 0 and 1 of philox4x32-10(counter = (j lo, j hi, t lo, t hi), key = (seed lo, seed hi)) as numpy's 53-bit double
__device__ __forceinline__ double philox_uniform(uint64_t seed, uint64_t j, uint64_t t) {
    uint32_t c0 = (uint32_t)j, c1 = (uint32_t)(j >> 32), c2 = (uint32_t)t, c3 = (uint32_t)(t >> 32);
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(kPhiloxM0, c0), lo0 = kPhiloxM0 * c0;
        const uint32_t hi1 = __umulhi(kPhiloxM1, c2), lo1 = kPhiloxM1 * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += kPhiloxW0;
        k1 += kPhiloxW1;
    }
    // (w0 >> 5) * 2^26 + (w1 >> 6) < 2^53: an integer, exact in fp64; the scaling is a power of two
    const uint64_t m = ((uint64_t)(c0 >> 5) << 26) | (uint64_t)(c1 >> 6);
    return (double)m * 0x1.0p-53;
}

struct Rule {
    const uint64_t* pts;        // [total,3] as bit patterns
    const int64_t* offsets;     // [B+1]
    int64_t total;
    int B;
    const double* desc;         // [B, SN_DESC_LEN] (null with SN_THIN_GROUP_NONE)
    int nx, ny, nz;
    int64_t G;                  // thresholds per tile
    const double* thr;          // [B, G]
    const double* u;            // [total] | null
    const uint64_t* seed;       // [1] | null
    const int64_t* tile_ids;    // [B] | null
};

// 64-bit atomic min, sent only where it would lower the slot (a stale look is a larger value: nothing is lost)
__device__ __forceinline__ void first_min(unsigned long long* slot, unsigned long long j) {
    if (__hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > j)
        __hip_atomic_fetch_min(slot, j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The decision of the chunk's rows: bit g of `keep` / `unb` is row base + g * 64 + lane's.  Rows of no tile (outside
// offsets[0] .. offsets[B]) and rows past `total` are neither.  key[g]: the row's group (kKey), -1 where it has none.
// first (kFirst): atomic min of the in-tile index over every BINNED row of a group, kept or not.
template <int kGroup, bool kKey, bool kFirst>
__device__ __forceinline__ void decide_chunk(const Rule& R, int64_t base, int lane, double* edges, uint32_t& keep,
                                             uint32_t& unb, int (&key)[kWaveGroups], unsigned long long* __restrict__ first) {
    keep = 0u;
    unb = 0u;
    if (kKey) {
#pragma unroll
        for (int g = 0; g < kWaveGroups; ++g) key[g] = -1;
    }
    const int64_t end = base + kWaveChunk < R.total ? base + kWaveChunk : R.total;
    const uint64_t seed = R.seed ? *R.seed : 0ull;
    const int ne = R.nx + R.ny + R.nz + 3;
    const int plane = R.nx * R.ny;
    // sn::for_tiles (packed_rows.h) written out: through it thin_count_kernel<SN_THIN_GROUP_VOXEL> takes 130 VGPRs, not 128,
    // and runs 3 waves per SIMD, not 4
    for (int b = sn::tile_of(R.offsets, R.B, base); b < R.B; ++b) {
        const int64_t lo = R.offsets[b], hi = R.offsets[b + 1];
        if (lo >= end) break;
        const int64_t from = lo > base ? lo : base, to = hi < end ? hi : end;
        if (from >= to) continue;   // an empty tile, or one that ends before the chunk
        sn::Binner bin;
        if (kGroup != SN_THIN_GROUP_NONE) {
            const double* d = R.desc + (size_t)b * (size_t)(6 + ne);
            __syncthreads();   // the previous tile's table has been read
            sn::load_edges(edges, d, ne, kWaveLanes);
            bin.init(edges, d, R.nx, R.ny, R.nz);
        }
        const uint64_t t = R.tile_ids ? (uint64_t)R.tile_ids[b] : (uint64_t)b;
        const double* thr = R.thr + (size_t)b * (size_t)R.G;
        unsigned long long* fst = kFirst && first ? first + (size_t)b * (size_t)R.G : nullptr;
        // `first` of the z rule: the wave's rows meet in nz words of LDS first, and one lane per slab takes the tile's
        // share to memory ([measured] 10^7 rows looking at the same 64 words of memory: 7x the count without `first`)
        unsigned long long* lfirst = reinterpret_cast<unsigned long long*>(edges + ne);
        if (kFirst && kGroup == SN_THIN_GROUP_Z && fst) {
            for (int k = lane; k < R.nz; k += kWaveLanes) lfirst[k] = ~0ull;
            __syncthreads();
        }
        // without groups the tile's first row is its row 0: the one lane that holds it says so
        if (kFirst && kGroup == SN_THIN_GROUP_NONE && fst && lo >= base && (int)((lo - base) & (kWaveLanes - 1)) == lane)
            fst[0] = 0ull;
#pragma unroll
        for (int g = 0; g < kWaveGroups; ++g) {
            const int64_t i = base + g * kWaveLanes + lane;
            if (i < from || i >= to) continue;
            int grp = 0;
            if (kGroup != SN_THIN_GROUP_NONE) {
                const uint64_t* p = R.pts + i * 3;
                const int f = bin.flat(__longlong_as_double((long long)p[0]), __longlong_as_double((long long)p[1]),
                                       __longlong_as_double((long long)p[2]));
                if (f < 0) {
                    unb |= 1u << g;
                    continue;
                }
                grp = kGroup == SN_THIN_GROUP_Z ? f / plane : f;
            }
            const uint64_t j = (uint64_t)(i - lo);
            const double uu = R.u ? R.u[i] : philox_uniform(seed, j, t);
            if (uu <= thr[grp]) keep |= 1u << g;
            if (kKey) key[g] = grp;
            if (kFirst && kGroup == SN_THIN_GROUP_Z && fst)
                __hip_atomic_fetch_min(lfirst + grp, (unsigned long long)j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            if (kFirst && kGroup == SN_THIN_GROUP_VOXEL && fst) first_min(fst + grp, j);
        }
        if (kFirst && kGroup == SN_THIN_GROUP_Z && fst) {
            __syncthreads();
            for (int k = lane; k < R.nz; k += kWaveLanes)
                if (lfirst[k] != ~0ull) first_min(fst + k, lfirst[k]);
        }
    }
}

// the workspace: kept[nchunks + 1], lost[nchunks + 1], keep[nchunks][16], unb[nchunks][16] -- 64-bit words
struct Ws {
    int64_t* kept;
    int64_t* lost;
    uint64_t* keep;
    uint64_t* unb;
};
__host__ __device__ inline Ws ws_of(void* ws, int64_t nchunks) {
    int64_t* w = static_cast<int64_t*>(ws);
    Ws r;
    r.kept = w;
    r.lost = w + (nchunks + 1);
    r.keep = reinterpret_cast<uint64_t*>(w + 2 * (nchunks + 1));
    r.unb = r.keep + nchunks * kWaveGroups;
    return r;
}

template <int kGroup>
__global__ __launch_bounds__(kWaveLanes) void thin_count_kernel(Rule R, int64_t nchunks, void* __restrict__ ws_raw,
                                                            unsigned long long* __restrict__ first) {
    extern __shared__ double edges[];
    const int lane = threadIdx.x;
    const int64_t chunk = blockIdx.x;
    uint32_t keep, unb;
    int key[kWaveGroups];
    decide_chunk<kGroup, false, true>(R, chunk * kWaveChunk, lane, edges, keep, unb, key, first);
    uint64_t mine_keep = 0, mine_unb = 0;
    int nkeep = 0, nunb = 0;
#pragma unroll
    for (int g = 0; g < kWaveGroups; ++g) {
        const unsigned long long mk = __ballot((keep >> g) & 1u), mu = __ballot((unb >> g) & 1u);
        nkeep += __popcll(mk);
        nunb += __popcll(mu);
        if (lane == g) {
            mine_keep = mk;
            mine_unb = mu;
        }
    }
    const Ws w = ws_of(ws_raw, nchunks);
    if (lane < kWaveGroups) {
        w.keep[chunk * kWaveGroups + lane] = mine_keep;
        w.unb[chunk * kWaveGroups + lane] = mine_unb;
    }
    if (lane == 0) {
        w.kept[chunk] = nkeep;
        w.lost[chunk] = nunb;
    }
}

// workgroup r (0: kept, 1: lost): row[0 .. nchunks) counts -> exclusive prefixes, row[nchunks] = the total
__global__ __launch_bounds__(kScanThreads) void thin_prefix_kernel(int64_t* __restrict__ ws, int64_t nchunks) {
    __shared__ int64_t s_wave[kScanThreads / 64];
    int64_t* row = ws + (int64_t)blockIdx.x * (nchunks + 1);
    const int64_t total = sn::scan_row<kScanThreads, kScanItems>(row, nchunks, s_wave);
    if (threadIdx.x == 0) row[nchunks] = total;
}

// set bits of `mask` [nchunks][16] in front of packed index p (clamped to 0 .. total), given the chunks' prefixes
__device__ __forceinline__ int64_t bits_before(const int64_t* __restrict__ prefix, const uint64_t* __restrict__ mask,
                                               int64_t nchunks, int64_t total, int64_t p) {
    p = p < 0 ? 0 : (p > total ? total : p);
    const int64_t c = p / kWaveChunk;
    if (c >= nchunks) return prefix[nchunks];   // p == total on a chunk seam
    const int r = (int)(p - c * kWaveChunk), full = r >> 6, rest = r & 63;
    int64_t n = prefix[c];
    const uint64_t* m = mask + c * kWaveGroups;
    for (int q = 0; q < full; ++q) n += __popcll(m[q]);
    if (rest) n += __popcll(m[full] & ((1ull << rest) - 1ull));
    return n;
}

// thread b of 0 .. B: offsets_out[b] = rows kept in front of offsets[b]; unbinned[b] = unbinned rows of tile b
__global__ __launch_bounds__(kScanThreads) void thin_offsets_kernel(const int64_t* __restrict__ offsets, int B, int64_t total,
                                                                    int64_t nchunks, void* __restrict__ ws_raw,
                                                                    int64_t* __restrict__ offsets_out,
                                                                    int64_t* __restrict__ unbinned) {
    const int b = blockIdx.x * kScanThreads + threadIdx.x;
    if (b > B) return;
    const Ws w = ws_of(ws_raw, nchunks);
    const int64_t p = offsets[b];
    offsets_out[b] = bits_before(w.kept, w.keep, nchunks, total, p);
    if (b < B)
        unbinned[b] = bits_before(w.lost, w.unb, nchunks, total, offsets[b + 1]) - bits_before(w.lost, w.unb, nchunks, total, p);
}

// kDecide: the decision is made again (and the groups found for out_key); otherwise the count's ballots are read
template <int kGroup, bool kDecide>
__global__ __launch_bounds__(kWaveLanes) void thin_scatter_kernel(Rule R, const uint64_t* __restrict__ labels, int64_t nchunks,
                                                              void* __restrict__ ws_raw, int64_t capacity,
                                                              uint64_t* __restrict__ out_pts, uint64_t* __restrict__ out_labels,
                                                              int64_t* __restrict__ out_src, int32_t* __restrict__ out_key) {
    extern __shared__ double edges[];
    const int lane = threadIdx.x;
    const int64_t chunk = blockIdx.x, base = chunk * kWaveChunk;
    const Ws w = ws_of(ws_raw, nchunks);
    uint32_t keep = 0u, unb = 0u;
    int key[kWaveGroups];
    if (kDecide) decide_chunk<kGroup, true, false>(R, base, lane, edges, keep, unb, key, nullptr);
    int64_t row = w.kept[chunk];
#pragma unroll
    for (int g = 0; g < kWaveGroups; ++g) {
        const unsigned long long mask = kDecide ? __ballot((keep >> g) & 1u) : w.keep[chunk * kWaveGroups + g];
        if ((mask >> lane) & 1ull) {
            const int64_t o = row + sn::wave_rank(mask);
            const int64_t i = base + g * kWaveLanes + lane;
            // (both tests also keep a workspace that is not this call's inside the buffers)
            if ((uint64_t)o < (uint64_t)capacity && i < R.total) {
                const uint64_t* p = R.pts + i * 3;
                uint64_t* q = out_pts + o * 3;
                q[0] = p[0];
                q[1] = p[1];
                q[2] = p[2];
                if (out_labels) out_labels[o] = labels[i];
                if (out_src) out_src[o] = i;
                if (out_key) out_key[o] = kDecide ? key[g] : 0;
            }
        }
        row += __popcll(mask);
    }
}

int64_t host_nchunks(int64_t total) { return (total + kWaveChunk - 1) / kWaveChunk; }
bool shape_served(int64_t total, int B) { return total > 0 && B > 0 && total <= kMaxTotal && B <= kMaxB; }

// the checks both entries share; `what` names the entry in the error text.  On SN_OK `R` is filled and `lds` set.
int check_common(const char* what, const double* pts, const int64_t* offsets, int64_t total, int B, int group,
                 const double* desc, int nx, int ny, int nz, const double* thr, const double* u, const uint64_t* seed,
                 const int64_t* tile_ids, const void* ws, size_t ws_bytes, Rule& R, size_t& lds) {
    if (!pts) return sn::fail(SN_ERR_INVALID_ARG, "%s: pts is null", what);
    if (!offsets) return sn::fail(SN_ERR_INVALID_ARG, "%s: offsets is null", what);
    if (!thr) return sn::fail(SN_ERR_INVALID_ARG, "%s: thr is null", what);
    if (!ws) return sn::fail(SN_ERR_INVALID_ARG, "%s: ws is null", what);
    if (total <= 0) return sn::fail(SN_ERR_INVALID_ARG, "%s: total must be positive (got %lld)", what, (long long)total);
    if (B <= 0) return sn::fail(SN_ERR_INVALID_ARG, "%s: B must be positive (got %d)", what, B);
    if (group != SN_THIN_GROUP_NONE && group != SN_THIN_GROUP_Z && group != SN_THIN_GROUP_VOXEL)
        return sn::fail(SN_ERR_INVALID_ARG, "%s: unknown group kind %d", what, group);
    if ((u == nullptr) == (seed == nullptr))
        return sn::fail(SN_ERR_INVALID_ARG, "%s: exactly one of u and seed is given", what);
    int64_t G = 1;
    lds = 0;
    if (group != SN_THIN_GROUP_NONE) {
        if (!desc) return sn::fail(SN_ERR_INVALID_ARG, "%s: group kind %d needs a descriptor", what, group);
        if (nx <= 0 || ny <= 0 || nz <= 0)
            return sn::fail(SN_ERR_INVALID_ARG, "%s: non-positive grid extent (%d, %d, %d)", what, nx, ny, nz);
    }
    if (!shape_served(total, B))
        return sn::fail(SN_ERR_UNSUPPORTED, "%s: total=%lld, B=%d beyond what is served (total <= 2^33, B <= %d)", what,
                        (long long)total, B, kMaxB);
    if (group != SN_THIN_GROUP_NONE) {
        // the edge tables, and behind them the z rule's nz words of `first`
        lds = ((size_t)nx + (size_t)ny + (size_t)nz + 3 + (group == SN_THIN_GROUP_Z ? (size_t)nz : 0)) * sizeof(double);
        if (lds > 64 * 1024) return sn::fail(SN_ERR_UNSUPPORTED, "%s: edge tables beyond 64 KiB of LDS", what);
        if ((int64_t)nx * ny * nz >= ((int64_t)1 << 31))
            return sn::fail(SN_ERR_UNSUPPORTED, "%s: nx * ny * nz >= 2^31", what);
        G = group == SN_THIN_GROUP_Z ? nz : (int64_t)nx * ny * nz;
    }
    if (ws_bytes < sn_thin_ws_bytes(total, B))
        return sn::fail(SN_ERR_INVALID_ARG, "%s: workspace of %zu bytes, sn_thin_ws_bytes asks for %zu", what, ws_bytes,
                        sn_thin_ws_bytes(total, B));
    if ((uintptr_t)pts % 8 || (uintptr_t)offsets % 8 || (uintptr_t)desc % 8 || (uintptr_t)thr % 8 || (uintptr_t)u % 8 ||
        (uintptr_t)seed % 8 || (uintptr_t)tile_ids % 8 || (uintptr_t)ws % 8)
        return sn::fail(SN_ERR_INVALID_ARG, "%s: pts / offsets / desc / thr / u / seed / tile_ids / ws must be 8-byte aligned",
                        what);
    R.pts = reinterpret_cast<const uint64_t*>(pts);
    R.offsets = offsets;
    R.total = total;
    R.B = B;
    R.desc = group != SN_THIN_GROUP_NONE ? desc : nullptr;
    R.nx = group != SN_THIN_GROUP_NONE ? nx : 0;
    R.ny = group != SN_THIN_GROUP_NONE ? ny : 0;
    R.nz = group != SN_THIN_GROUP_NONE ? nz : 0;
    R.G = G;
    R.thr = thr;
    R.u = u;
    R.seed = seed;
    R.tile_ids = tile_ids;
    return SN_OK;
}

}  // namespace

extern "C" size_t sn_thin_ws_bytes(int64_t total, int B) {
    if (!shape_served(total, B)) return 0;
    const int64_t nchunks = host_nchunks(total);
    return (size_t)(2 * (nchunks + 1) + 2 * nchunks * kWaveGroups) * sizeof(int64_t);
}

extern "C" int sn_thin_chunk_points(void) { return kWaveChunk; }

extern "C" int sn_thin_count(const double* pts, const int64_t* offsets, int64_t total, int B, int group, const double* desc,
                             int nx, int ny, int nz, const double* thr, const double* u, const uint64_t* seed,
                             const int64_t* tile_ids, void* ws, size_t ws_bytes, int64_t* offsets_out, int64_t* unbinned,
                             uint64_t* first, sn_stream_t stream) {
    const char* what = "sn_thin_count";
    Rule R;
    size_t lds;
    const int rc = check_common(what, pts, offsets, total, B, group, desc, nx, ny, nz, thr, u, seed, tile_ids, ws, ws_bytes, R,
                                lds);
    if (rc != SN_OK) return rc;
    if (!offsets_out) return sn::fail(SN_ERR_INVALID_ARG, "%s: offsets_out is null", what);
    if (!unbinned) return sn::fail(SN_ERR_INVALID_ARG, "%s: unbinned is null", what);
    if ((uintptr_t)offsets_out % 8 || (uintptr_t)unbinned % 8 || (uintptr_t)first % 8)
        return sn::fail(SN_ERR_INVALID_ARG, "%s: offsets_out / unbinned / first must be 8-byte aligned", what);
    hipStream_t s = sn::as_stream(stream);
    if (first && hipMemsetAsync(first, 0xff, (size_t)B * (size_t)R.G * sizeof(uint64_t), s) != hipSuccess)
        return sn::fail(SN_ERR_LAUNCH, "%s: hipMemsetAsync failed", what);
    const int64_t nchunks = host_nchunks(total);
    unsigned long long* f = reinterpret_cast<unsigned long long*>(first);
    const dim3 grid((unsigned)nchunks), block(kWaveLanes);
    if (group == SN_THIN_GROUP_NONE)
        hipLaunchKernelGGL(thin_count_kernel<SN_THIN_GROUP_NONE>, grid, block, 0, s, R, nchunks, ws, f);
    else if (group == SN_THIN_GROUP_Z)
        hipLaunchKernelGGL(thin_count_kernel<SN_THIN_GROUP_Z>, grid, block, lds, s, R, nchunks, ws, f);
    else
        hipLaunchKernelGGL(thin_count_kernel<SN_THIN_GROUP_VOXEL>, grid, block, lds, s, R, nchunks, ws, f);
    hipLaunchKernelGGL(thin_prefix_kernel, dim3(2), dim3(kScanThreads), 0, s, static_cast<int64_t*>(ws), nchunks);
    hipLaunchKernelGGL(thin_offsets_kernel, dim3((unsigned)(B / kScanThreads + 1)), dim3(kScanThreads), 0, s, offsets, B, total,
                       nchunks, ws, offsets_out, unbinned);
    return sn::check_launch(what);
}

extern "C" int sn_thin_scatter(const double* pts, const double* labels, const int64_t* offsets, int64_t total, int B, int group,
                               const double* desc, int nx, int ny, int nz, const double* thr, const double* u,
                               const uint64_t* seed, const int64_t* tile_ids, const void* ws, size_t ws_bytes, int64_t capacity, double* out_pts, double* out_labels, int64_t* out_src, int32_t* out_key,
                               sn_stream_t stream) {
    const char* what = "sn_thin_scatter";
    Rule R;
    size_t lds;
    const int rc = check_common(what, pts, offsets, total, B, group, desc, nx, ny, nz, thr, u, seed, tile_ids, ws, ws_bytes, R,
                                lds);
    if (rc != SN_OK) return rc;
    if (!out_pts) return sn::fail(SN_ERR_INVALID_ARG, "%s: out_pts is null", what);
    if (capacity < 0) return sn::fail(SN_ERR_INVALID_ARG, "%s: capacity must not be negative (got %lld)", what, (long long)capacity);
    if ((labels == nullptr) != (out_labels == nullptr))
        return sn::fail(SN_ERR_INVALID_ARG, "%s: out_labels is given iff labels is", what);
    if ((uintptr_t)labels % 8 || (uintptr_t)out_pts % 8 || (uintptr_t)out_labels % 8 || (uintptr_t)out_src % 8 ||
        (uintptr_t)out_key % 4)
        return sn::fail(SN_ERR_INVALID_ARG, "%s: labels / out_pts / out_labels / out_src must be 8-byte, out_key 4-byte aligned",
                        what);
    const int64_t nchunks = host_nchunks(total);
    hipStream_t s = sn::as_stream(stream);
    const dim3 grid((unsigned)nchunks), block(kWaveLanes);
    void* w = const_cast<void*>(ws);   // (read only: ws_of serves both kernels)
    const uint64_t* lab = reinterpret_cast<const uint64_t*>(labels);
    uint64_t* op = reinterpret_cast<uint64_t*>(out_pts);
    uint64_t* ol = reinterpret_cast<uint64_t*>(out_labels);
    // without groups every key is 0: nothing to decide for it
    const bool decide = out_key != nullptr && group != SN_THIN_GROUP_NONE;
#define SN_THIN_SCATTER(GROUP, DECIDE, LDS)                                                                              \
    hipLaunchKernelGGL((thin_scatter_kernel<GROUP, DECIDE>), grid, block, LDS, s, R, lab, nchunks, w, capacity, op, ol, \
                       out_src, out_key)
    if (!decide) SN_THIN_SCATTER(SN_THIN_GROUP_NONE, false, 0);
    else if (group == SN_THIN_GROUP_Z) SN_THIN_SCATTER(SN_THIN_GROUP_Z, true, lds);
    else SN_THIN_SCATTER(SN_THIN_GROUP_VOXEL, true, lds);
#undef SN_THIN_SCATTER
    return sn::check_launch(what);
}
