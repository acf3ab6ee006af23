// K9 -- scan crops: K disc / box regions cut out of one scan into a CSR batch of K tiles (sn_crop_count, sn_crop_scatter).
// replaces: the host-side crops of utils/pcd_processing.py -- crop_at_locations (:820-840), crop_tower_radius (:666-697),
//           crop_two_towers (:700-739), crop_tower_samples (:805-817, driven by core/datasets/ts40k.py:31-148
//           build_data_samples): each an `a[mask]` over the whole cloud per centre, with an np.append of the label column.
//
// Definition (normative, include/scenenet_hip.h): a disc row (cx, cy, r, -) holds point i iff
// (x-cx)*(x-cx) + (y-cy)*(y-cy) <= r*r, every product and the sum rounded once in fp64 (this file is built with
// -ffp-contract=off: a fused dx*dx + fl(dy*dy) differs from numpy's value in about one draw in eight around a UTM centre);
// a box row (xmin, ymin, xmax, ymax) iff xmin <= x && x <= xmax && ymin <= y && y <= ymax.  The comparisons are taken
// literally (a NaN anywhere is false).  Tile k holds region k's members in scan order; x, y, z and the label travel as
// 64-bit patterns.
//
// Shape: one WAVE per workgroup and kWaveChunk = 1024 consecutive points per workgroup -- lane l holds x, y of the points
// chunk * 1024 + g * 64 + l, g = 0..15, in registers (64 VGPRs).  A workgroup of one wave has nobody to exchange with: no
// LDS, no barrier.  Regions are outermost: lane l fetches row k0 + l of a tile of 64 regions with one vector load each, and
// the row travels to the wave's scalar registers by v_readlane (a wave-uniform value per region, one fetch per 1024 points).
// Per region and group __ballot of the membership gives the wave-uniform __popcll (count) and, in the scatter, the lane's
// rank by mbcnt of the same mask: output order is scan order by construction, nothing depends on scheduling.
//   count:   ws[k][chunk] = members of region k in the chunk (int64, one slot per (region, workgroup): no memset, no atomics)
//   prefix:  one workgroup per region turns its row into exclusive prefixes, total in ws[k][nchunks]
//   offsets: one workgroup, the exclusive prefix of the totals
//   scatter: recomputes the test, but only for the regions whose slot says the chunk holds a member (an exact skip: the
//            count is the count of the very same test) -- a region far from the chunk costs two loads per 64 regions.
// Chunk-level reject in the count pass: the wave reduces its chunk's xy box (NaN coordinates left out: they are in no
// region), every lane tests the box against ITS region of the tile (cannot_reach: conservative by construction, proof at
// the function), and only the regions the box can reach are looped over; the others' slots get 0.
//
// Bound: the two passes read 24 B per point each (x, y, z share their cache lines), the scatter 8 B more per member for the
// label and writes 32..40 B per member; per region and point 8 fp64 VALU operations.  HBM-bound up to K of a few dozen,
// VALU-bound beyond.
#include "common.h"
#include "scan.h"
#include "regions.h"   // Region, load_region, broadcast, member, cannot_reach, wave_min_max, load_xy: shared with K19

namespace {

__global__ __launch_bounds__(kWaveLanes) void crop_count_kernel(const uint64_t* __restrict__ pts, int64_t n,
                                                            const double* __restrict__ regions,
                                                            const int32_t* __restrict__ kinds, int K, int64_t nchunks,
                                                            int64_t* __restrict__ ws) {
    const int lane = threadIdx.x;
    const int64_t chunk = blockIdx.x;
    uint64_t x[kWaveGroups], y[kWaveGroups];
    load_xy(pts, n, chunk * kWaveChunk, lane, x, y);
    double xlo, xhi, ylo, yhi;
    wave_min_max(x, xlo, xhi);
    wave_min_max(y, ylo, yhi);
    for (int k0 = 0; k0 < K; k0 += kWaveLanes) {
        const Region mine = load_region(regions, kinds, K, k0 + lane);   // (k >= K: kind -1, out of reach)
        unsigned long long live = __ballot(!cannot_reach(mine, xlo, xhi, ylo, yhi));
        int mycount = 0;
        while (live) {
            const int j = __ffsll(live) - 1;
            live &= live - 1;
            const Region R = broadcast(mine, j);
            int cnt = 0;
#pragma unroll
            for (int g = 0; g < kWaveGroups; ++g)
                cnt += __popcll(__ballot(member(R, __longlong_as_double((long long)x[g]), __longlong_as_double((long long)y[g]))));
            if (lane == j) mycount = cnt;
        }
        if (k0 + lane < K) ws[(int64_t)(k0 + lane) * (nchunks + 1) + chunk] = mycount;
    }
}

// workgroup k: ws[k][0 .. nchunks) counts -> exclusive prefixes, ws[k][nchunks] = the region's total
__global__ __launch_bounds__(kScanThreads) void crop_prefix_kernel(int64_t* __restrict__ ws, int64_t nchunks) {
    __shared__ int64_t s_wave[kScanThreads / 64];
    int64_t* row = ws + (int64_t)blockIdx.x * (nchunks + 1);
    const int64_t total = sn::scan_row<kScanThreads, kScanItems>(row, nchunks, s_wave);
    if (threadIdx.x == 0) row[nchunks] = total;
}

// one workgroup: offsets[k] = members of the regions before k, offsets[K] = all
__global__ __launch_bounds__(kScanThreads) void crop_offsets_kernel(const int64_t* __restrict__ ws, int64_t nchunks, int K,
                                                                    int64_t* __restrict__ offsets) {
    __shared__ int64_t s_wave[kScanThreads / 64];
    sn::totals_to_offsets<kScanThreads>(ws, nchunks + 1, nchunks, K, offsets, s_wave);
}

// (waves_per_eu 3: left alone the allocator takes 170 VGPRs, two over the limit of three waves per SIMD; at 168 it still
// needs no scratch -- at four waves it would -- and the scatter, which waits on HBM, is 8-15 % faster on the part)
__global__ __launch_bounds__(kWaveLanes) __attribute__((amdgpu_waves_per_eu(3))) void crop_scatter_kernel(const uint64_t* __restrict__ pts,
                                                              const uint64_t* __restrict__ labels, int64_t n,
                                                              const double* __restrict__ regions,
                                                              const int32_t* __restrict__ kinds, int K, int64_t nchunks,
                                                              const int64_t* __restrict__ ws,
                                                              const int64_t* __restrict__ offsets, int64_t capacity,
                                                              uint64_t* __restrict__ out_pts, uint64_t* __restrict__ out_labels,
                                                              int64_t* __restrict__ out_src) {
    const int lane = threadIdx.x;
    const int64_t chunk = blockIdx.x, base = chunk * kWaveChunk;
    uint64_t x[kWaveGroups], y[kWaveGroups];
    load_xy(pts, n, base, lane, x, y);
    for (int k0 = 0; k0 < K; k0 += kWaveLanes) {
        const int k = k0 + lane;
        const Region mine = load_region(regions, kinds, K, k);
        int64_t myfirst = 0, mycount = 0;
        if (k < K) {
            const int64_t* slot = ws + (int64_t)k * (nchunks + 1) + chunk;
            const int64_t before = slot[0];
            mycount = slot[1] - before;      // (slot[1] of the last chunk is the region's total)
            myfirst = offsets[k] + before;
        }
        // regions with a member in this chunk, by the count pass's own test: the others are skipped exactly
        unsigned long long live = __ballot(mycount != 0);
        while (live) {
            const int j = __ffsll(live) - 1;
            live &= live - 1;
            const Region R = broadcast(mine, j);
            int64_t row = (int64_t)readlane64((uint64_t)myfirst, j);
#pragma unroll
            for (int g = 0; g < kWaveGroups; ++g) {
                const bool in = member(R, __longlong_as_double((long long)x[g]), __longlong_as_double((long long)y[g]));
                const unsigned long long mask = __ballot(in);
                if (in) {
                    const int64_t o = row + sn::wave_rank(mask);
                    if ((uint64_t)o < (uint64_t)capacity) {   // (also keeps a workspace that is not this call's inside the buffer)
                        const int64_t i = base + g * kWaveLanes + lane;
                        uint64_t* p = out_pts + o * 3;
                        p[0] = x[g];
                        p[1] = y[g];
                        p[2] = pts[i * 3 + 2];
                        if (out_labels) out_labels[o] = labels[i];
                        if (out_src) out_src[o] = i;
                    }
                }
                row += __popcll(mask);
            }
        }
    }
}

// ---- K12: the label census of the same regions (sn_crop_census) ---------------------------------------------------------
// Per region: members, members with a NaN label, members per watch range [lo, hi], smallest / largest non-NaN label --
// the membership test is member() above, the chunk-level reject cannot_reach(), the shape crop_count_kernel's.  What a
// chunk contributes to a region is reduced over the wave first (ballot + popcount land in scalar registers; min / max by
// six xor-shuffles) and then added to the region's row of ws by 64-bit integer atomics, only where it is not zero: integer
// sums and maxima commute, so the result does not depend on the order the workgroups arrive in.
//   ws[shard][k] = { n, n_nan, watch[0..C), ~enc(min), enc(max) }   all zero before the launch: ONE memset node
// Workgroup b adds to shard b % kCensusShards, the decode launch folds the shards: the workgroups that meet in one region
// (every 1024-point chunk inside a large box) would otherwise queue up on one cache line of atomics.  The two maxima are
// looked at first (a relaxed load) and the atomic is only sent where it would raise the slot -- a stale look is a smaller
// value, so nothing is lost -- which leaves one or two atomics per (region, chunk) once a region's range has settled.
// enc is common.h's order-preserving map (K1's) of an fp64 to a uint64 (-0.0 below +0.0); the minimum is kept as the maximum of
// the complement.  No non-NaN value encodes to 0 and none to ~0, so 0 says "no such member" in both slots.
// Per point the label is read once and turned into its code and a word of flags (bit c: inside watch range c, bit 31:
// NaN), before the region loop.  A group of 64 points without a member of the region (the usual case) costs the test and
// one ballot; the label work sits behind a scalar branch on that ballot.
constexpr uint32_t kLabelNaN = 1u << 31;
constexpr int kCensusShards = 8;

using sn::enc_f64;   // common.h: the encoding K1's boxes use
using sn::dec_f64;

template <bool kLabels>
__global__ __launch_bounds__(kWaveLanes) void crop_census_kernel(const uint64_t* __restrict__ pts,
                                                             const double* __restrict__ labels, int64_t n,
                                                             const double* __restrict__ regions,
                                                             const int32_t* __restrict__ kinds, int K,
                                                             const double* __restrict__ watch, int C,
                                                             unsigned long long* __restrict__ ws) {
    const int lane = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * kWaveChunk;
    const int S = C + 4;   // words per region
    uint64_t x[kWaveGroups], y[kWaveGroups];
    load_xy(pts, n, base, lane, x, y);
    uint64_t code[kWaveGroups];    // enc of the label; 0: NaN (or no label)
    uint32_t flags[kWaveGroups];
    if (kLabels) {
        // lane c holds watch range c; a lane without one holds (NaN, NaN): matches nothing, and is never asked for
        const double nan = __longlong_as_double((long long)kNaNBits);
        const double wlo = lane < C ? watch[2 * lane] : nan, whi = lane < C ? watch[2 * lane + 1] : nan;
#pragma unroll
        for (int g = 0; g < kWaveGroups; ++g) {
            const int64_t i = base + g * kWaveLanes + lane;
            const double l = i < n ? labels[i] : nan;   // (past the end: in no region, never counted)
            const bool isnan = l != l;
            code[g] = isnan ? 0ull : enc_f64(l);
            flags[g] = isnan ? kLabelNaN : 0u;
        }
        for (int c = 0; c < C; ++c) {
            const double lo = readlane_f64(wlo, c), hi = readlane_f64(whi, c);
#pragma unroll
            for (int g = 0; g < kWaveGroups; ++g) {
                const double l = dec_f64(code[g]);      // (code 0 decodes to a NaN: in no range)
                flags[g] |= (lo <= l && l <= hi) ? (1u << c) : 0u;
            }
        }
    }
    double xlo, xhi, ylo, yhi;
    wave_min_max(x, xlo, xhi);
    wave_min_max(y, ylo, yhi);
    for (int k0 = 0; k0 < K; k0 += kWaveLanes) {
        const Region mine = load_region(regions, kinds, K, k0 + lane);   // (k >= K: kind -1, out of reach)
        unsigned long long live = __ballot(!cannot_reach(mine, xlo, xhi, ylo, yhi));
        while (live) {
            const int j = __ffsll(live) - 1;
            live &= live - 1;
            const Region R = broadcast(mine, j);
            int cnt = 0, cnan = 0;
            uint64_t mine_val = 0;      // lane t: word t of the region's row, this chunk's share
            uint64_t vmax = 0, vminc = 0;
#pragma unroll
            for (int g = 0; g < kWaveGroups; ++g) {
                const bool in = member(R, __longlong_as_double((long long)x[g]), __longlong_as_double((long long)y[g]));
                const unsigned long long mask = __ballot(in);
                if (mask == 0) continue;
                cnt += __popcll(mask);
                if (kLabels) {
                    const uint32_t f = in ? flags[g] : 0u;
                    cnan += __popcll(__ballot((f & kLabelNaN) != 0));
                    for (int c = 0; c < C; ++c) {
                        const int w = __popcll(__ballot(((f >> c) & 1u) != 0));
                        if (lane == 2 + c) mine_val += (uint64_t)w;
                    }
                    const uint64_t e = in ? code[g] : 0ull;       // (a NaN label's code is 0: it moves neither end)
                    const uint64_t ec = e ? ~e : 0ull;
                    vmax = e > vmax ? e : vmax;
                    vminc = ec > vminc ? ec : vminc;
                }
            }
            if (cnt == 0) continue;
            if (lane == 0) mine_val = (uint64_t)cnt;
            if (lane == 1) mine_val = (uint64_t)cnan;
            if (kLabels && cnt != cnan) {
                const auto larger = [](uint64_t mine, uint64_t other) { return other > mine ? other : mine; };
                vmax = sn::wave_reduce(vmax, larger);
                vminc = sn::wave_reduce(vminc, larger);
                if (lane == 2 + C) mine_val = vminc;
                if (lane == 3 + C) mine_val = vmax;
            }
            if (lane < S && mine_val != 0) {
                const int shard = (int)(blockIdx.x % kCensusShards);
                unsigned long long* slot = ws + ((int64_t)shard * K + (k0 + j)) * S + lane;
                if (lane < 2 + C)
                    __hip_atomic_fetch_add(slot, (unsigned long long)mine_val, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                else if (__hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < mine_val)
                    __hip_atomic_fetch_max(slot, (unsigned long long)mine_val, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
}

// thread k: row k of every shard of ws -> counts[k][0 .. 2 + C) and, with labels, label_range[k] = (min, max) as plain fp64
__global__ __launch_bounds__(kScanThreads) void crop_census_decode_kernel(const unsigned long long* __restrict__ ws, int K, int C,
                                                                          int64_t* __restrict__ counts,
                                                                          double* __restrict__ label_range) {
    const int k = blockIdx.x * kScanThreads + threadIdx.x;
    if (k >= K) return;
    const int S = C + 4;
    const int64_t shard_words = (int64_t)K * S;
    const unsigned long long* row = ws + (int64_t)k * S;
    for (int t = 0; t < 2 + C; ++t) {
        unsigned long long sum = 0;
        for (int h = 0; h < kCensusShards; ++h) sum += row[h * shard_words + t];
        counts[(int64_t)k * (2 + C) + t] = (int64_t)sum;
    }
    if (label_range) {
        unsigned long long cmin = 0, emax = 0;
        for (int h = 0; h < kCensusShards; ++h) {
            const unsigned long long a = row[h * shard_words + 2 + C], b = row[h * shard_words + 3 + C];
            cmin = a > cmin ? a : cmin;
            emax = b > emax ? b : emax;
        }
        label_range[2 * (int64_t)k] = cmin ? dec_f64(~cmin) : __longlong_as_double(0x7ff0000000000000ll);
        label_range[2 * (int64_t)k + 1] = emax ? dec_f64(emax) : __longlong_as_double((long long)0xfff0000000000000ull);
    }
}

bool shape_served(int64_t n, int K) { return n > 0 && K > 0 && n <= kMaxN && K <= kMaxK; }
int64_t host_nchunks(int64_t n) { return (n + kWaveChunk - 1) / kWaveChunk; }

// the checks both entries share; `what` names the entry in the error text
int check_common(const char* what, const void* pts, int64_t n, const void* regions, const void* kinds, int K, const void* ws,
                 size_t ws_bytes, const void* offsets) {
    if (!pts) return sn::fail(SN_ERR_INVALID_ARG, "%s: pts is null", what);
    if (!regions) return sn::fail(SN_ERR_INVALID_ARG, "%s: regions is null", what);
    if (!ws) return sn::fail(SN_ERR_INVALID_ARG, "%s: ws is null", what);
    if (!offsets) return sn::fail(SN_ERR_INVALID_ARG, "%s: offsets is null", what);
    if (n <= 0) return sn::fail(SN_ERR_INVALID_ARG, "%s: n must be positive (got %lld)", what, (long long)n);
    if (K <= 0) return sn::fail(SN_ERR_INVALID_ARG, "%s: K must be positive (got %d)", what, K);
    if (!shape_served(n, K))
        return sn::fail(SN_ERR_UNSUPPORTED, "%s: n=%lld, K=%d beyond what is served (n <= 2^36, K <= %d)", what, (long long)n,
                        K, kMaxK);
    if (ws_bytes < sn_crops_ws_bytes(n, K))
        return sn::fail(SN_ERR_INVALID_ARG, "%s: workspace of %zu bytes, sn_crops_ws_bytes asks for %zu", what, ws_bytes,
                        sn_crops_ws_bytes(n, K));
    if ((uintptr_t)pts % 8 || (uintptr_t)regions % 8 || (uintptr_t)ws % 8 || (uintptr_t)offsets % 8 || (uintptr_t)kinds % 4)
        return sn::fail(SN_ERR_INVALID_ARG, "%s: pts / regions / ws / offsets must be 8-byte, kinds 4-byte aligned", what);
    return SN_OK;
}

}  // namespace

extern "C" size_t sn_crops_ws_bytes(int64_t n, int K) {
    if (!shape_served(n, K)) return 0;
    return (size_t)K * (size_t)(host_nchunks(n) + 1) * sizeof(int64_t);
}

extern "C" int sn_crops_chunk_points(void) { return kWaveChunk; }

extern "C" int sn_crop_count(const double* pts, int64_t n, const double* regions, const int32_t* kinds, int K, void* ws,
                             size_t ws_bytes, int64_t* offsets, sn_stream_t stream) {
    const int rc = check_common("sn_crop_count", pts, n, regions, kinds, K, ws, ws_bytes, offsets);
    if (rc != SN_OK) return rc;
    hipStream_t s = sn::as_stream(stream);
    const int64_t nchunks = host_nchunks(n);
    int64_t* w = static_cast<int64_t*>(ws);
    hipLaunchKernelGGL(crop_count_kernel, dim3((unsigned)nchunks), dim3(kWaveLanes), 0, s,
                       reinterpret_cast<const uint64_t*>(pts), n, regions, kinds, K, nchunks, w);
    hipLaunchKernelGGL(crop_prefix_kernel, dim3((unsigned)K), dim3(kScanThreads), 0, s, w, nchunks);
    hipLaunchKernelGGL(crop_offsets_kernel, dim3(1), dim3(kScanThreads), 0, s, w, nchunks, K, offsets);
    return sn::check_launch("sn_crop_count");
}

extern "C" int sn_crop_scatter(const double* pts, const double* labels, int64_t n, const double* regions,
                               const int32_t* kinds, int K, const void* ws, size_t ws_bytes, const int64_t* offsets,
                               int64_t capacity, double* out_pts, double* out_labels, int64_t* out_src, sn_stream_t stream) {
    const int rc = check_common("sn_crop_scatter", pts, n, regions, kinds, K, ws, ws_bytes, offsets);
    if (rc != SN_OK) return rc;
    if (!out_pts) return sn::fail(SN_ERR_INVALID_ARG, "sn_crop_scatter: out_pts is null");
    if (capacity < 0)
        return sn::fail(SN_ERR_INVALID_ARG, "sn_crop_scatter: capacity must not be negative (got %lld)", (long long)capacity);
    if ((labels == nullptr) != (out_labels == nullptr))
        return sn::fail(SN_ERR_INVALID_ARG, "sn_crop_scatter: out_labels is given iff labels is");
    if ((uintptr_t)labels % 8 || (uintptr_t)out_pts % 8 || (uintptr_t)out_labels % 8 || (uintptr_t)out_src % 8)
        return sn::fail(SN_ERR_INVALID_ARG, "sn_crop_scatter: labels / out_pts / out_labels / out_src must be 8-byte aligned");
    const int64_t nchunks = host_nchunks(n);
    hipLaunchKernelGGL(crop_scatter_kernel, dim3((unsigned)nchunks), dim3(kWaveLanes), 0, sn::as_stream(stream),
                       reinterpret_cast<const uint64_t*>(pts), reinterpret_cast<const uint64_t*>(labels), n, regions, kinds, K,
                       nchunks, static_cast<const int64_t*>(ws), offsets, capacity, reinterpret_cast<uint64_t*>(out_pts),
                       reinterpret_cast<uint64_t*>(out_labels), out_src);
    return sn::check_launch("sn_crop_scatter");
}

namespace {
bool census_served(int64_t n, int K, int C) { return shape_served(n, K) && C >= 0 && C <= SN_CENSUS_MAX_WATCH; }
}  // namespace

extern "C" size_t sn_crop_census_ws_bytes(int64_t n, int K, int C) {
    if (!census_served(n, K, C)) return 0;
    return (size_t)kCensusShards * (size_t)K * (size_t)(C + 4) * sizeof(uint64_t);
}

extern "C" int sn_census_chunk_points(void) { return kWaveChunk; }

extern "C" int sn_crop_census(const double* pts, const double* labels, int64_t n, const double* regions, const int32_t* kinds,
                              int K, const double* watch, int C, void* ws, size_t ws_bytes, int64_t* counts,
                              double* label_range, sn_stream_t stream) {
    const char* what = "sn_crop_census";
    if (!pts) return sn::fail(SN_ERR_INVALID_ARG, "%s: pts is null", what);
    if (!regions) return sn::fail(SN_ERR_INVALID_ARG, "%s: regions is null", what);
    if (!ws) return sn::fail(SN_ERR_INVALID_ARG, "%s: ws is null", what);
    if (!counts) return sn::fail(SN_ERR_INVALID_ARG, "%s: counts is null", what);
    if (n <= 0) return sn::fail(SN_ERR_INVALID_ARG, "%s: n must be positive (got %lld)", what, (long long)n);
    if (K <= 0) return sn::fail(SN_ERR_INVALID_ARG, "%s: K must be positive (got %d)", what, K);
    if (C < 0) return sn::fail(SN_ERR_INVALID_ARG, "%s: C must not be negative (got %d)", what, C);
    if (!census_served(n, K, C))
        return sn::fail(SN_ERR_UNSUPPORTED, "%s: n=%lld, K=%d, C=%d beyond what is served (n <= 2^36, K <= %d, C <= %d)", what,
                        (long long)n, K, C, kMaxK, SN_CENSUS_MAX_WATCH);
    if (C > 0 && !labels) return sn::fail(SN_ERR_INVALID_ARG, "%s: C=%d watch ranges without labels", what, C);
    if ((watch == nullptr) != (C == 0)) return sn::fail(SN_ERR_INVALID_ARG, "%s: watch is given iff C > 0", what);
    if ((labels == nullptr) != (label_range == nullptr))
        return sn::fail(SN_ERR_INVALID_ARG, "%s: label_range is given iff labels is", what);
    if (ws_bytes < sn_crop_census_ws_bytes(n, K, C))
        return sn::fail(SN_ERR_INVALID_ARG, "%s: workspace of %zu bytes, sn_crop_census_ws_bytes asks for %zu", what, ws_bytes,
                        sn_crop_census_ws_bytes(n, K, C));
    if ((uintptr_t)pts % 8 || (uintptr_t)labels % 8 || (uintptr_t)regions % 8 || (uintptr_t)watch % 8 || (uintptr_t)ws % 8 ||
        (uintptr_t)counts % 8 || (uintptr_t)label_range % 8 || (uintptr_t)kinds % 4)
        return sn::fail(SN_ERR_INVALID_ARG,
                        "%s: pts / labels / regions / watch / ws / counts / label_range must be 8-byte, kinds 4-byte aligned", what);
    hipStream_t s = sn::as_stream(stream);
    unsigned long long* w = static_cast<unsigned long long*>(ws);
    if (hipMemsetAsync(w, 0, sn_crop_census_ws_bytes(n, K, C), s) != hipSuccess)
        return sn::fail(SN_ERR_LAUNCH, "%s: hipMemsetAsync failed", what);
    const int64_t nchunks = host_nchunks(n);
    if (labels)
        hipLaunchKernelGGL(crop_census_kernel<true>, dim3((unsigned)nchunks), dim3(kWaveLanes), 0, s,
                           reinterpret_cast<const uint64_t*>(pts), labels, n, regions, kinds, K, watch, C, w);
    else
        hipLaunchKernelGGL(crop_census_kernel<false>, dim3((unsigned)nchunks), dim3(kWaveLanes), 0, s,
                           reinterpret_cast<const uint64_t*>(pts), labels, n, regions, kinds, K, watch, C, w);
    hipLaunchKernelGGL(crop_census_decode_kernel, dim3((unsigned)((K + kScanThreads - 1) / kScanThreads)), dim3(kScanThreads), 0, s,
                       w, K, C, counts, label_range);
    return sn::check_launch(what);
}
