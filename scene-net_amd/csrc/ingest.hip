// K7 -- tile ingest: raw rows of B concatenated tiles -> the pts [total,3] / labels [total] layout that K1 and
// sn_gather_points take (sn_tiles_unpack).
// replaces: the host-side split of a sample, core/datasets/ts40k.py:201-207 (`npy = np.load(...)`,
//           `sample = (npy[:, 0:-1], npy[:, -1])`), which the reference runs once per sample in 8 DataLoader workers; here
//           the file's rows travel host-to-device as they are and are de-interleaved where the bandwidth is.
//
// Values are moved as bit patterns: an f64 row is copied word for word (NaN payloads, -0.0, denormals unchanged); an f32
// row is widened with integer arithmetic only (exact for every finite value and infinity; a NaN keeps its sign and payload
// and gets the quiet bit, as an IEEE conversion gives), so the result does not depend on the floating-point mode.
// `bad` counts, per tile, the points with a non-finite value in a column that is read: the common point tests its
// exponent fields and does nothing more; a non-finite one finds its tile by a binary search of offsets and adds 1 with an
// integer atomic (bad is cleared by a memset node ahead of the kernel: written, not accumulated; integer adds do not
// depend on order).
//
// Bound: HBM.  Algorithmic bytes per point: cols * sizeof(row element) read, 24 (+ 8 with labels) written -- 64 B at
// four f64 columns.  Two forms: cols == 4 with rows / pts / labels 16-byte aligned moves a PAIR of points per lane with
// 16-byte loads and stores (two rows are 64 or 32 contiguous bytes, their points 48, their labels 16; an odd last point
// goes alone); any other shape or alignment moves one point per lane with element-sized accesses, which need no more than
// element alignment (rows are only element-aligned when cols is odd).
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 2048;   // grid-stride beyond (256 CUs x 8 workgroups)

struct alignas(16) U64x2 {
    uint64_t a, b;
};
struct alignas(16) U32x4 {
    uint32_t a, b, c, d;
};

__device__ __forceinline__ uint64_t widen_bits(uint64_t v) { return v; }
__device__ __forceinline__ uint64_t widen_bits(uint32_t u) { return sn::widen_f32_bits(u); }
__device__ __forceinline__ bool nonfinite(uint64_t v) { return (v & 0x7ff0000000000000ull) == 0x7ff0000000000000ull; }

// tile of point i: offsets[b] <= i < offsets[b + 1]; stays inside [0, B) whatever offsets holds
__device__ __forceinline__ void count_bad(int64_t i, const int64_t* __restrict__ offsets, int B, int32_t* bad) {
    int lo = 0, hi = B;
    while (hi - lo > 1) {
        const int mid = lo + ((hi - lo) >> 1);
        if (offsets[mid] <= i) lo = mid; else hi = mid;
    }
    atomicAdd(&bad[lo], 1);
}

template <typename W>   // W: uint64_t (f64 rows) | uint32_t (f32 rows)
__device__ __forceinline__ void unpack_point(const W* __restrict__ rows, int cols, int64_t i, const int64_t* offsets, int B,
                                             uint64_t* __restrict__ pts, uint64_t* __restrict__ labels, int32_t* bad) {
    const W* r = rows + i * (int64_t)cols;
    const uint64_t x = widen_bits(r[0]), y = widen_bits(r[1]), z = widen_bits(r[2]);
    uint64_t* p = pts + i * 3;
    p[0] = x;
    p[1] = y;
    p[2] = z;
    bool nf = nonfinite(x) || nonfinite(y) || nonfinite(z);
    if (labels) {
        const uint64_t l = widen_bits(r[cols - 1]);
        labels[i] = l;
        nf = nf || nonfinite(l);
    }
    if (bad && nf) count_bad(i, offsets, B, bad);
}

// any cols, element-aligned pointers: one point per lane
template <typename W>
__global__ __launch_bounds__(kThreads) void tiles_unpack_rows_kernel(const W* __restrict__ rows, int cols, int64_t total,
                                                                     const int64_t* __restrict__ offsets, int B,
                                                                     uint64_t* __restrict__ pts,
                                                                     uint64_t* __restrict__ labels,
                                                                     int32_t* __restrict__ bad) {
    const int64_t stride = (int64_t)gridDim.x * kThreads;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += stride)
        unpack_point<W>(rows, cols, i, offsets, B, pts, labels, bad);
}

template <typename W> struct PairLoad;
template <> struct PairLoad<uint64_t> {   // rows 2k, 2k+1: 64 bytes
    static __device__ __forceinline__ void load(const uint64_t* r, uint64_t (&v)[8]) {
        const U64x2* q = reinterpret_cast<const U64x2*>(r);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const U64x2 u = q[k];
            v[2 * k] = u.a;
            v[2 * k + 1] = u.b;
        }
    }
};
template <> struct PairLoad<uint32_t> {   // 32 bytes
    static __device__ __forceinline__ void load(const uint32_t* r, uint64_t (&v)[8]) {
        const U32x4* q = reinterpret_cast<const U32x4*>(r);
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const U32x4 u = q[k];
            v[4 * k] = widen_bits(u.a);
            v[4 * k + 1] = widen_bits(u.b);
            v[4 * k + 2] = widen_bits(u.c);
            v[4 * k + 3] = widen_bits(u.d);
        }
    }
};

// cols == 4, rows / pts / labels 16-byte aligned: points 2k and 2k+1 per lane, 16-byte accesses only
template <typename W>
__global__ __launch_bounds__(kThreads) void tiles_unpack_pairs_kernel(const W* __restrict__ rows, int64_t total,
                                                                      const int64_t* __restrict__ offsets, int B,
                                                                      uint64_t* __restrict__ pts,
                                                                      uint64_t* __restrict__ labels,
                                                                      int32_t* __restrict__ bad) {
    const int64_t pairs = total >> 1, stride = (int64_t)gridDim.x * kThreads;
    for (int64_t k = (int64_t)blockIdx.x * kThreads + threadIdx.x; k < pairs; k += stride) {
        uint64_t v[8];
        PairLoad<W>::load(rows + k * 8, v);
        U64x2* p = reinterpret_cast<U64x2*>(pts + k * 6);
        p[0] = U64x2{v[0], v[1]};
        p[1] = U64x2{v[2], v[4]};
        p[2] = U64x2{v[5], v[6]};
        bool nf0 = nonfinite(v[0]) || nonfinite(v[1]) || nonfinite(v[2]);
        bool nf1 = nonfinite(v[4]) || nonfinite(v[5]) || nonfinite(v[6]);
        if (labels) {
            *reinterpret_cast<U64x2*>(labels + k * 2) = U64x2{v[3], v[7]};
            nf0 = nf0 || nonfinite(v[3]);
            nf1 = nf1 || nonfinite(v[7]);
        }
        if (bad) {
            if (nf0) count_bad(2 * k, offsets, B, bad);
            if (nf1) count_bad(2 * k + 1, offsets, B, bad);
        }
    }
    if ((total & 1) && blockIdx.x == 0 && threadIdx.x == 0)
        unpack_point<W>(rows, 4, total - 1, offsets, B, pts, labels, bad);
}

template <typename W>
void launch_unpack(const void* rows, int cols, int64_t total, const int64_t* offsets, int B, double* pts, double* labels,
                   int32_t* bad, hipStream_t s) {
    const W* r = static_cast<const W*>(rows);
    uint64_t* p = reinterpret_cast<uint64_t*>(pts);
    uint64_t* l = reinterpret_cast<uint64_t*>(labels);
    const bool aligned = ((uintptr_t)rows % 16 == 0) && ((uintptr_t)pts % 16 == 0) && ((uintptr_t)labels % 16 == 0);
    const int64_t work = (cols == 4 && aligned) ? (total + 1) / 2 : total;
    const int64_t want = (work + kThreads - 1) / kThreads;
    const dim3 grid((unsigned)(want < kMaxBlocks ? want : kMaxBlocks)), block(kThreads);
    if (cols == 4 && aligned)
        hipLaunchKernelGGL(tiles_unpack_pairs_kernel<W>, grid, block, 0, s, r, total, offsets, B, p, l, bad);
    else
        hipLaunchKernelGGL(tiles_unpack_rows_kernel<W>, grid, block, 0, s, r, cols, total, offsets, B, p, l, bad);
}

}  // namespace

extern "C" int sn_tiles_unpack(const void* rows, int row_dtype, int cols, int64_t total, const int64_t* offsets, int B,
                               double* pts, double* labels, int32_t* bad, sn_stream_t stream) {
    if (!rows) return sn::fail(SN_ERR_INVALID_ARG, "sn_tiles_unpack: rows is null");
    if (!pts) return sn::fail(SN_ERR_INVALID_ARG, "sn_tiles_unpack: pts is null");
    if (total <= 0) return sn::fail(SN_ERR_INVALID_ARG, "sn_tiles_unpack: total must be positive (got %lld)", (long long)total);
    if (B <= 0) return sn::fail(SN_ERR_INVALID_ARG, "sn_tiles_unpack: B must be positive (got %d)", B);
    if (cols < 3 || cols > 8) return sn::fail(SN_ERR_INVALID_ARG, "sn_tiles_unpack: cols must lie in 3..8 (got cols=%d)", cols);
    if (labels && cols == 3)
        return sn::fail(SN_ERR_INVALID_ARG, "sn_tiles_unpack: labels need cols >= 4 (rows of cols=3 hold x, y, z only)");
    if (bad && !offsets) return sn::fail(SN_ERR_INVALID_ARG, "sn_tiles_unpack: bad needs offsets");
    if (row_dtype != SN_F32 && row_dtype != SN_F64) {
        if (row_dtype == SN_U8 || row_dtype == SN_OCC8 || row_dtype == SN_BF16 || row_dtype == SN_I32)
            return sn::fail(SN_ERR_UNSUPPORTED, "sn_tiles_unpack: row_dtype %d is not served (SN_F32 | SN_F64)", row_dtype);
        return sn::fail(SN_ERR_INVALID_ARG, "sn_tiles_unpack: unknown row_dtype %d", row_dtype);
    }
    const size_t esz = row_dtype == SN_F64 ? 8 : 4;
    if ((uintptr_t)rows % esz) return sn::fail(SN_ERR_INVALID_ARG, "sn_tiles_unpack: rows must be aligned to its element size");
    if ((uintptr_t)pts % 8 || (uintptr_t)labels % 8 || (uintptr_t)offsets % 8 || (uintptr_t)bad % 4)
        return sn::fail(SN_ERR_INVALID_ARG, "sn_tiles_unpack: pts / labels / offsets must be 8-byte, bad 4-byte aligned");
    hipStream_t s = sn::as_stream(stream);
    if (bad) {
        const hipError_t e = hipMemsetAsync(bad, 0, (size_t)B * sizeof(int32_t), s);
        if (e != hipSuccess) return sn::fail(SN_ERR_LAUNCH, "sn_tiles_unpack(clear bad): %s", hipGetErrorString(e));
    }
    if (row_dtype == SN_F64)
        launch_unpack<uint64_t>(rows, cols, total, offsets, B, pts, labels, bad, s);
    else
        launch_unpack<uint32_t>(rows, cols, total, offsets, B, pts, labels, bad, s);
    return sn::check_launch("sn_tiles_unpack");
}
