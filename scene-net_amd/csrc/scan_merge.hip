// K19 -- scan merge: the predictions of K tiles put back on the whole scan in one pass (sn_scan_merge).
// replaces: the last step of the whole-scan recipe -- sn_gather_points over the cropped rows (one value per ROW of the
//           crops), then crops.merge_to_scan's five torch launches (full(-inf), scatter_reduce_(amax) through fp atomics,
//           zeros, an index put, where) over the crops' src column.  The reference has no whole-scan step at all.
//
// Definition (normative, include/scenenet_hip.h): region k covers point i iff k has a tile (0 <= tile_of[k] < B), the point
// is a member of k by K9's test (regions.h: the same text) and it bins inside that tile's edge table by sn_gather_points'
// rule (binning.h: the same text; a size-mode padding cell is outside).  cover[i] counts the covering regions; a point with
// none reads `fill`.  MAX: the largest covering value, NaN if one is NaN.  MEAN: the fp64 sum in ascending region index,
// divided by the count, rounded to the grid's type.  INTERIOR: the value of the covering region the point lies deepest in
// (depth in the region's own geometry; the first covering region is held, a later one replaces it iff its depth > the held
// one, so ties go to the lowest index).
//
// Shape: K9's count kernel.  One WAVE per workgroup and kWaveChunk = 1024 consecutive points per workgroup, x and y of 16
// groups of 64 points in registers; regions outermost, 64 at a time, one per lane, the chunk's xy box against the lane's
// region (cannot_reach), the live ones broadcast to scalar registers one after the other.  ONE thread owns one scan point:
// its count and its accumulator (a value, an fp64 sum, or a depth and a value) stay in registers from the first region to
// the last, so there are no atomics, no workspace and nothing to initialise, and the order of combination is the region
// order whatever the scheduling.  A live region's membership is evaluated for the 16 groups first (one bit per group in a
// lane's word); only if the chunk holds a member are the nx + ny + nz + 3 edges of its tile brought into LDS (1.5 KB at 64^3;
// one wave: the barriers around the copy cost no wait for another wave), and only the groups with a member bin and read
// the grid.  The chunk's z waits in LDS behind the edges (8 KB, written once at the start; where table and z do not fit
// 64 KiB together a member loads its z from memory instead), and a region's groups are taken eight at a time in three
// sweeps -- bin, read the grid, combine -- so that eight grid reads are in flight together.  [measured, 10^7 points, 128
// boxes of 30 m with 5 m overlap, nine regions per chunk] the first form loaded z from memory and binned, read and combined
// group after group, one memory latency after the other: 574 us (rule max); this form 386 us.
// Channels ride on gridDim.y: a channel beyond the first repeats the tests, which keeps the registers of one accumulator
// per point whatever C is (the model has one channel).
//
// Bound: 24 B read per point, 4 B (f32) written, 4 B more with cover, one grid read per covering region; per live region
// and point 8 fp64 operations, per member the six LDS reads of Binner::flat.  With one region per chunk the kernel runs at
// the two reads it fuses; with many overlapping regions per chunk the per-region work -- an edge table
// into LDS, 16 group sweeps in which only the members' lanes work -- is what it waits for.
#include "common.h"
#include "scan.h"
#include "regions.h"
#include "binning.h"

namespace {

using sn::Binner;
constexpr int kHalf = kWaveGroups / 2;   // groups whose grid reads are in flight together

// a < b ? a : b, literally: the depth's minimum (no operand is NaN for a member with finite bounds; where one is, this is
// the text the header states)
__device__ __forceinline__ double lesser(double a, double b) { return a < b ? a : b; }

// how deep a member (x, y) of R lies inside it: every operation rounded once (-ffp-contract=off), both roots correctly rounded
__device__ __forceinline__ double depth_in(const Region& R, double x, double y) {
#pragma clang fp contract(off)
    if (R.kind == SN_CROP_DISC) {
        const double dx = x - R.a, dy = y - R.b;
        const double xx = dx * dx, yy = dy * dy;
        const double s = xx + yy;                    // the number the membership test compares with R.c = fl(r*r)
        return __dsqrt_rn(R.c) - __dsqrt_rn(s);
    }
    return lesser(lesser(x - R.a, R.c - x), lesser(y - R.b, R.d - y));
}

template <typename T, int kRule>
struct Acc;
template <typename T>
struct Acc<T, SN_MERGE_MAX> {
    T v;
    __device__ __forceinline__ void first(T a, double) { v = a; }
    __device__ __forceinline__ void next(T a, double) { v = (a > v || a != a) ? a : v; }   // (a held NaN stays: both false)
    __device__ __forceinline__ T result(int) const { return v; }
};
template <typename T>
struct Acc<T, SN_MERGE_MEAN> {
    double s;
    __device__ __forceinline__ void first(T a, double) { s = (double)a; }
    __device__ __forceinline__ void next(T a, double) { s = s + (double)a; }
    __device__ __forceinline__ T result(int cnt) const { return (T)(s / (double)cnt); }
};
template <typename T>
struct Acc<T, SN_MERGE_INTERIOR> {
    T v;
    double d;
    __device__ __forceinline__ void first(T a, double dep) { v = a; d = dep; }
    __device__ __forceinline__ void next(T a, double dep) {
        if (dep > d) { v = a; d = dep; }
    }
    __device__ __forceinline__ T result(int) const { return v; }
};

template <typename T, int kRule>
__global__ __launch_bounds__(kWaveLanes) void scan_merge_kernel(const T* __restrict__ grid, int channels, int B, int nx, int ny,
                                                            int nz, const double* __restrict__ desc,
                                                            const uint64_t* __restrict__ pts, int64_t n,
                                                            const double* __restrict__ regions,
                                                            const int32_t* __restrict__ kinds,
                                                            const int32_t* __restrict__ tile_of, int K, T fill,
                                                            T* __restrict__ out, int32_t* __restrict__ cover, int z_in_lds) {
    extern __shared__ double edges[];
    const int lane = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * kWaveChunk;
    const int c = blockIdx.y;
    const int ne = nx + ny + nz + 3;
    const int64_t V = (int64_t)nx * ny * nz;
    uint64_t x[kWaveGroups], y[kWaveGroups];
    load_xy(pts, n, base, lane, x, y);
    // z of the chunk waits in LDS behind the edge table (8 KB; its cache lines come with x and y): a member reads it once
    // per covering region, and a read from memory there costs a latency each time.  (Visible after the barrier in front
    // of the first use, the one that follows the copy of the edges.)
    double* zs = z_in_lds ? edges + ne : nullptr;
    if (zs) {
#pragma unroll
        for (int g = 0; g < kWaveGroups; ++g) {
            const int64_t i = base + g * kWaveLanes + lane;
            zs[g * kWaveLanes + lane] = __longlong_as_double((long long)(i < n ? pts[i * 3 + 2] : kNaNBits));
        }
    }
    double xlo, xhi, ylo, yhi;
    wave_min_max(x, xlo, xhi);
    wave_min_max(y, ylo, yhi);
    int cnt[kWaveGroups];
    Acc<T, kRule> acc[kWaveGroups];
#pragma unroll
    for (int g = 0; g < kWaveGroups; ++g) {
        cnt[g] = 0;
        acc[g].first((T)0, 0.0);
    }
    for (int k0 = 0; k0 < K; k0 += kWaveLanes) {
        const int k = k0 + lane;
        const Region mine = load_region(regions, kinds, K, k);   // (k >= K: kind -1, out of reach)
        const int mytile = k < K ? (tile_of ? tile_of[k] : k) : -1;
        // a region without a tile covers nothing; the others are looped over if the chunk's box can reach them
        unsigned long long live = __ballot((unsigned)mytile < (unsigned)B && !cannot_reach(mine, xlo, xhi, ylo, yhi));
        while (live) {
            const int j = __ffsll(live) - 1;
            live &= live - 1;
            const Region R = broadcast(mine, j);
            const int t = __builtin_amdgcn_readlane(mytile, j);
            uint32_t mbits = 0;      // bit g: this lane's point of group g is a member
#pragma unroll
            for (int g = 0; g < kWaveGroups; ++g)
                mbits |= member(R, __longlong_as_double((long long)x[g]), __longlong_as_double((long long)y[g])) ? (1u << g) : 0u;
            if (__ballot(mbits != 0) == 0) continue;
            const double* d = desc + (int64_t)t * (6 + ne);
            __syncthreads();         // (one wave: orders the last region's LDS reads before this copy, no wait for anybody)
            sn::load_edges(edges, d, ne, kWaveLanes);
            Binner bin;
            bin.init(edges, d, nx, ny, nz);
            // a size-mode table is padded with +inf edges beyond the tile's own n_a: the padding cells are outside
            // (gather_points_kernel's rule, voxel.hip)
            const bool padded = !(bin.ex[nx] <= DBL_MAX && bin.ey[ny] <= DBL_MAX && bin.ez[nz] <= DBL_MAX);
            const T* gt = grid + ((int64_t)t * channels + c) * V;
            // half a chunk at a time, in three sweeps, so that the eight grid reads of a half are in flight together (a
            // sweep that binned, read and combined group after group waited out one memory latency per group and region)
#pragma unroll
            for (int h = 0; h < kWaveGroups; h += kHalf) {
                int f[kHalf];
#pragma unroll
                for (int q = 0; q < kHalf; ++q) {
                    const int g = h + q;
                    const bool in = (mbits >> g) & 1u;
                    f[q] = -1;
                    if (__ballot(in) == 0) continue;
                    if (in) {
                        const int64_t i = base + g * kWaveLanes + lane;      // (a member: i < n)
                        const double xv = __longlong_as_double((long long)x[g]), yv = __longlong_as_double((long long)y[g]);
                        const double zv = zs ? zs[g * kWaveLanes + lane] : __longlong_as_double((long long)pts[i * 3 + 2]);
                        int fl = bin.flat(xv, yv, zv);
                        if (padded && fl >= 0) {
                            const int r = fl / ny, iy = fl - r * ny, iz = r / nx, ix = r - iz * nx;
                            if (!(bin.ex[ix + 1] <= DBL_MAX && bin.ey[iy + 1] <= DBL_MAX && bin.ez[iz + 1] <= DBL_MAX)) fl = -1;
                        }
                        f[q] = fl;
                    }
                }
                T v[kHalf];
#pragma unroll
                for (int q = 0; q < kHalf; ++q) v[q] = f[q] >= 0 ? gt[f[q]] : (T)0;
#pragma unroll
                for (int q = 0; q < kHalf; ++q) {
                    const int g = h + q;
                    if (f[q] >= 0) {
                        const double dep = kRule == SN_MERGE_INTERIOR
                                               ? depth_in(R, __longlong_as_double((long long)x[g]), __longlong_as_double((long long)y[g]))
                                               : 0.0;
                        if (cnt[g] == 0) acc[g].first(v[q], dep);
                        else acc[g].next(v[q], dep);
                        ++cnt[g];
                    }
                }
            }
        }
    }
    T* o = out + (int64_t)c * n;
#pragma unroll
    for (int g = 0; g < kWaveGroups; ++g) {
        const int64_t i = base + g * kWaveLanes + lane;
        if (i < n) {
            o[i] = cnt[g] ? acc[g].result(cnt[g]) : fill;
            if (cover && c == 0) cover[i] = cnt[g];
        }
    }
}

template <typename T>
void launch(int rule, dim3 grd, size_t lds, hipStream_t s, const void* grid, int channels, int B, int nx, int ny, int nz,
            const double* desc, const double* pts, int64_t n, const double* regions, const int32_t* kinds,
            const int32_t* tile_of, int K, double fill, void* out, int32_t* cover, int z_in_lds) {
#define SN_MERGE(RULE)                                                                                                   \
    hipLaunchKernelGGL((scan_merge_kernel<T, RULE>), grd, dim3(kWaveLanes), lds, s, (const T*)grid, channels, B, nx, ny, nz, \
                       desc, reinterpret_cast<const uint64_t*>(pts), n, regions, kinds, tile_of, K, (T)fill, (T*)out, cover, \
                       z_in_lds)
    if (rule == SN_MERGE_MAX) SN_MERGE(SN_MERGE_MAX);
    else if (rule == SN_MERGE_MEAN) SN_MERGE(SN_MERGE_MEAN);
    else SN_MERGE(SN_MERGE_INTERIOR);
#undef SN_MERGE
}

}  // namespace

extern "C" int sn_scan_merge(const void* grid, int dtype, int channels, int B, int nx, int ny, int nz, const double* desc,
                             const double* pts, int64_t n, const double* regions, const int32_t* kinds,
                             const int32_t* tile_of, int K, int rule, double fill, void* out, int32_t* cover,
                             sn_stream_t stream) {
    const char* what = "sn_scan_merge";
    if (!grid) return sn::fail(SN_ERR_INVALID_ARG, "%s: grid is null", what);
    if (!desc) return sn::fail(SN_ERR_INVALID_ARG, "%s: desc is null", what);
    if (!pts) return sn::fail(SN_ERR_INVALID_ARG, "%s: pts is null", what);
    if (!regions) return sn::fail(SN_ERR_INVALID_ARG, "%s: regions is null", what);
    if (!out) return sn::fail(SN_ERR_INVALID_ARG, "%s: out is null", what);
    if (n <= 0) return sn::fail(SN_ERR_INVALID_ARG, "%s: n must be positive (got %lld)", what, (long long)n);
    if (K <= 0) return sn::fail(SN_ERR_INVALID_ARG, "%s: K must be positive (got %d)", what, K);
    if (B <= 0 || channels <= 0 || nx <= 0 || ny <= 0 || nz <= 0)
        return sn::fail(SN_ERR_INVALID_ARG, "%s: non-positive extent (B=%d, channels=%d, grid %d x %d x %d)", what, B, channels,
                        nx, ny, nz);
    if (rule != SN_MERGE_MAX && rule != SN_MERGE_MEAN && rule != SN_MERGE_INTERIOR)
        return sn::fail(SN_ERR_INVALID_ARG, "%s: rule %d (SN_MERGE_MAX | SN_MERGE_MEAN | SN_MERGE_INTERIOR)", what, rule);
    if (dtype != SN_F32 && dtype != SN_F64) return sn::fail(SN_ERR_INVALID_ARG, "%s: dtype %d (SN_F32 | SN_F64)", what, dtype);
    if (!tile_of && B != K)
        return sn::fail(SN_ERR_INVALID_ARG, "%s: without tile_of region k reads tile k: B=%d must equal K=%d", what, B, K);
    const uintptr_t esize = dtype == SN_F32 ? 4 : 8;
    if ((uintptr_t)pts % 8 || (uintptr_t)regions % 8 || (uintptr_t)desc % 8 || (uintptr_t)kinds % 4 || (uintptr_t)tile_of % 4 ||
        (uintptr_t)cover % 4 || (uintptr_t)grid % esize || (uintptr_t)out % esize)
        return sn::fail(SN_ERR_INVALID_ARG,
                        "%s: pts / regions / desc must be 8-byte, kinds / tile_of / cover 4-byte, grid / out element aligned", what);
    if (n > kMaxN || K > kMaxK)
        return sn::fail(SN_ERR_UNSUPPORTED, "%s: n=%lld, K=%d beyond what is served (n <= 2^36, K <= %d)", what, (long long)n, K,
                        kMaxK);
    if (channels > 65535)
        return sn::fail(SN_ERR_UNSUPPORTED, "%s: channels=%d beyond what is served (<= 65535: they ride on gridDim.y)", what,
                        channels);
    size_t lds = ((size_t)nx + (size_t)ny + (size_t)nz + 3) * sizeof(double);
    if (lds > 64 * 1024) return sn::fail(SN_ERR_UNSUPPORTED, "%s: edge table > 64 KiB", what);
    // the chunk's z rides in LDS behind the edges where both fit 64 KiB (always, short of a table of 7000 edges)
    const int z_in_lds = lds + kWaveChunk * sizeof(double) <= 64 * 1024;
    if (z_in_lds) lds += kWaveChunk * sizeof(double);
    const int64_t nchunks = (n + kWaveChunk - 1) / kWaveChunk;
    const dim3 grd((unsigned)nchunks, (unsigned)channels);
    hipStream_t s = sn::as_stream(stream);
    if (dtype == SN_F32)
        launch<float>(rule, grd, lds, s, grid, channels, B, nx, ny, nz, desc, pts, n, regions, kinds, tile_of, K, fill, out, cover,
                      z_in_lds);
    else
        launch<double>(rule, grd, lds, s, grid, channels, B, nx, ny, nz, desc, pts, n, regions, kinds, tile_of, K, fill, out,
                       cover, z_in_lds);
    return sn::check_launch(what);
}
