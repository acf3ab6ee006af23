// K13 -- LAS decode: the point records of an uncompressed .las file -> pts [n,3] f64, classes [n] f64 and a class histogram
// (sn_las_decode).
// replaces: utils/pcd_processing.py:99-120 las_to_numpy behind lp.read(filename), core/datasets/ts40k.py:73-86 -- laspy's
//           scaled views (three int32 columns times scale plus offset, in fp64, on one host core), np.vstack(...).transpose()
//           (a strided copy of the whole scan) and np.array(las.classification); only then could the scan be uploaded.
//           Here the file's record bytes travel host-to-device as they are and are decoded where the bandwidth is.
//
// Definition (normative, include/scenenet_hip.h).  A record is record_length bytes, little-endian.  X, Y, Z are int32 at
// bytes 0, 4, 8;  pts[i] = (fl(fl((double)X * sx) + ox), ...) -- the conversion is exact, the product and the sum are
// rounded once each and never contracted (this file is built with -ffp-contract=off): numpy's `X * scale + offset`.
// The class is byte 15 & 31 for the point formats 0..5 and byte 16 for 6..10.  hist[c] GAINS the number of records of
// class c.  No other byte of a record is interpreted.
//
// Shape.  One workgroup of 256 lanes decodes kChunk = 256 records at a time, one record per lane, and walks the chunks
// c = blockIdx.x, blockIdx.x + gridDim.x, ... (the grid is capped at kMaxBlocks, so a workgroup's histogram stays in LDS
// over all its chunks and is flushed once).  `records` has ANY byte alignment and record_length is rarely a multiple of 4,
// so no lane's fields are aligned in global memory.  Two ways to the five dwords that hold a record's bytes 0..16:
//   staged (record_length <= kMaxStagedStride, every standard length and then some): the chunk's byte span is loaded as
//          aligned 16-byte granules by consecutive lanes (1 KiB per wave-instruction) into REGISTERS one pass ahead --
//          2, 3, 4 or 6 granules per lane, by record length --, goes to LDS at the start of its own pass, and while the
//          lanes read the five ALIGNED LDS dwords around their records and funnel-shift the fields out of them
//          (v_alignbyte_b32) the next chunk's loads are in flight.  The staging area is dynamic LDS sized by the record
//          length (8 KiB at 20..31 bytes), so that eight workgroups fit a CU.
//          [measured, 10^7 points, before / after the loads ran one pass ahead with LDS sized by the record length:
//          157 -> 119 us at 28 B, 159 -> 134 us at 34 B; the first form took the same time at every record length]
//   direct (longer records: most of the span is not needed, and a lane's 17 bytes share no cache line with its
//          neighbour's): the same five aligned dwords, read from global memory.
// Neither form issues a byte-wide global load.  Both leave a chunk's results in LDS as the chunk's part of pts / classes
// will lie in memory, and the workgroup stores that image with 16-byte stores -- an 8-byte one at either end where the
// chunk's part starts or ends on an odd multiple of 8.  Per chunk: two barriers.
//
// Bound: HBM.  Algorithmic bytes per point: record_length read, 24 + 8 written -- 60 B at format 1, 66 at format 3.
// LDS per point, staged: record_length written and 20 read as dwords, 32 written and read for the output image.  Lane i
// reads LDS at a stride of record_length bytes: conflict-free for odd dword strides (28 B = 7 dwords), up to 8-way for 32 B.
#include "common.h"
#include <cmath>

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kChunk = 256;             // records per workgroup and pass: one per lane
constexpr int kMaxBlocks = 2048;        // 256 CUs x 8 workgroups; further chunks are walked
constexpr int kMaxStagedStride = 80;    // the longest standard record is 67 bytes (format 10)
constexpr int64_t kMaxRecords = (int64_t)1 << 36;             // a workgroup's LDS histogram counts in 32 bits

typedef uint32_t U32x4 __attribute__((ext_vector_type(4)));   // 16 bytes, 16-byte aligned
typedef double F64x2 __attribute__((ext_vector_type(2)));

struct LasShape {
    int64_t n;
    int stride;        // record_length
    int class_byte;    // 15 | 16
    uint32_t class_mask;   // 31 | 255
    double scale[3], offset[3];
};

// bytes k..k+3 of the eight bytes (lo, hi), k in 0..3: v_alignbyte_b32
__device__ __forceinline__ uint32_t bytes_at(uint32_t hi, uint32_t lo, uint32_t k) {
    return __builtin_amdgcn_alignbyte(hi, lo, k);
}

// what the staged form keeps in registers for the NEXT chunk: NG granules per lane, lane t those at t, t + 256, ...
template <int NG>
struct Prefetch {
    U32x4 v[NG > 0 ? NG : 1];
    int head, granules;
    // The span's bytes [span, span + cnt * stride) are brought in as the aligned 16-byte granules that hold them.  The
    // first and the last granule may reach up to 15 bytes in front of the first record and behind the last one, bytes that
    // are not the caller's.  READING them is safe: an aligned 16-byte granule never straddles a page (pages are multiples
    // of 16 bytes), and each of the two holds at least one valid byte, so it lies in a page that is mapped for the span.
    // They are never written, and what was read from them is never used: a lane's five dwords start at the dword that
    // holds its record's byte 0 and end at the one that holds byte 16 <= record_length - 1 (record_length >= 20 is
    // checked by the entry, >= 30 where byte 16 is the class), except for the at most 3 bytes in front of byte 0 in d[0]
    // and behind byte 16 in d[4], which bytes_at() shifts out.
    // (A lane without a granule of its own loads the span's last one again: always a granule of the span.)
    __device__ __forceinline__ void issue(const uint8_t* span, int cnt, int stride, int t) {
        head = (int)(reinterpret_cast<uintptr_t>(span) & 15);
        granules = (head + cnt * stride + 15) >> 4;   // <= NG * kThreads (the entry picks NG)
        const U32x4* src = reinterpret_cast<const U32x4*>(span - head);
        const int last = granules - 1;
#pragma unroll
        for (int j = 0; j < NG; ++j) {
            const int g = t + j * kThreads;
            v[j] = src[g < last ? g : last];
        }
    }
    __device__ __forceinline__ void to_lds(U32x4* stage, int t) const {
#pragma unroll
        for (int j = 0; j < NG; ++j) {
            const int g = t + j * kThreads;
            if (g < granules) stage[g] = v[j];
        }
    }
};

// NG > 0: the staged form, NG granules per lane and chunk (dynamic LDS: NG * kThreads granules); NG == 0: the direct form
template <int NG>
__global__ __launch_bounds__(kThreads) void las_decode_kernel(const uint8_t* __restrict__ records, LasShape sh,
                                                              double* __restrict__ pts, double* __restrict__ classes,
                                                              unsigned long long* __restrict__ hist) {
    constexpr bool kStaged = NG > 0;
    __shared__ F64x2 out_pts[kChunk * 3 / 2];
    __shared__ F64x2 out_cls[kChunk / 2];
    __shared__ uint32_t bins[256];
    extern __shared__ U32x4 stage[];   // (the static arrays above are 9216 bytes: the dynamic part starts 16-byte aligned)
    const int t = threadIdx.x;
    if (hist) bins[t] = 0;   // (kThreads == 256; ordered ahead of the first add by the chunk's first barrier)
    const int64_t chunks = (sh.n + kChunk - 1) / kChunk;
    const uint32_t* stage_words = reinterpret_cast<const uint32_t*>(stage);
    double* lds_pts = reinterpret_cast<double*>(out_pts);
    double* lds_cls = reinterpret_cast<double*>(out_cls);
    Prefetch<NG> pre;
    if (kStaged) {   // (gridDim.x <= chunks: every workgroup has a first chunk)
        const int64_t first = (int64_t)blockIdx.x * kChunk;
        pre.issue(records + first * (int64_t)sh.stride, (int)((sh.n - first) < kChunk ? (sh.n - first) : kChunk), sh.stride, t);
    }

    for (int64_t c = blockIdx.x; c < chunks; c += gridDim.x) {
        const int64_t first = c * kChunk;
        const int cnt = (int)((sh.n - first) < kChunk ? (sh.n - first) : kChunk);
        const uint8_t* span = records + first * (int64_t)sh.stride;   // 64-bit: n * record_length may pass 2^31
        uint32_t d[5] = {0, 0, 0, 0, 0};
        uint32_t k = 0;
        if (kStaged) {
            // this chunk's granules wait in registers since the previous pass: to LDS, and while the lanes decode from
            // there and store the image, the next chunk's loads are in flight
            const int head = pre.head;
            pre.to_lds(stage, t);
            __syncthreads();
            const int64_t next = (c + gridDim.x) * kChunk;
            if (next < sh.n)
                pre.issue(records + next * (int64_t)sh.stride, (int)((sh.n - next) < kChunk ? (sh.n - next) : kChunk), sh.stride, t);
            if (t < cnt) {
                const int o = head + t * sh.stride;   // the record's byte 0 in the staged image
                k = (uint32_t)o & 3u;
                const uint32_t* w = stage_words + (o >> 2);
#pragma unroll
                for (int j = 0; j < 5; ++j) d[j] = w[j];
            }
        } else {
            __syncthreads();   // (the image of the previous chunk has been stored by every lane)
            if (t < cnt) {
                // The five aligned dwords from byte 0's to byte 16's: the first may reach up to 3 bytes in front of the
                // record -- for the span's first record bytes that are not the caller's, in the aligned granule (hence the
                // page) of a valid byte, as argued at Prefetch; the last ends at or before the record's byte 19.
                const uint8_t* a = span + (int64_t)t * sh.stride;
                k = (uint32_t)reinterpret_cast<uintptr_t>(a) & 3u;
                const uint32_t* w = reinterpret_cast<const uint32_t*>(a - k);
#pragma unroll
                for (int j = 0; j < 5; ++j) d[j] = w[j];
            }
        }
        if (t < cnt) {
            const int32_t X = (int32_t)bytes_at(d[1], d[0], k);
            const int32_t Y = (int32_t)bytes_at(d[2], d[1], k);
            const int32_t Z = (int32_t)bytes_at(d[3], d[2], k);
            // byte 16 is byte k of d[4]; byte 15 is the last of the four from byte 12
            const uint32_t raw = sh.class_byte == 16 ? (d[4] >> (8 * k)) : (bytes_at(d[4], d[3], k) >> 24);
            const uint32_t cls = raw & sh.class_mask;
            lds_pts[3 * t + 0] = (double)X * sh.scale[0] + sh.offset[0];
            lds_pts[3 * t + 1] = (double)Y * sh.scale[1] + sh.offset[1];
            lds_pts[3 * t + 2] = (double)Z * sh.scale[2] + sh.offset[2];
            lds_cls[t] = (double)cls;
            if (hist) atomicAdd(&bins[cls], 1u);
        }
        __syncthreads();
        // the chunk's image: 3 * cnt doubles of pts from pts + 3 * first, cnt doubles of classes from classes + first; a
        // lane stores pairs that are 16-byte aligned in MEMORY, lanes 0 and 1 the single doubles at the two ends
        {
            double* g = pts + 3 * first;
            const int m = 3 * cnt;
            const int lead = (int)((reinterpret_cast<uintptr_t>(g) >> 3) & 1);   // (m >= 3 > lead)
            const int pairs = (m - lead) >> 1;
            for (int j = t; j < pairs; j += kThreads)
                *reinterpret_cast<F64x2*>(g + lead + 2 * j) = F64x2{lds_pts[lead + 2 * j], lds_pts[lead + 2 * j + 1]};
            if (t == 0 && lead) g[0] = lds_pts[0];
            if (t == 1 && ((m - lead) & 1)) g[m - 1] = lds_pts[m - 1];
        }
        if (classes) {
            double* g = classes + first;
            const int lead = (int)((reinterpret_cast<uintptr_t>(g) >> 3) & 1);   // cnt == 1 with lead: no pair, no tail
            const int pairs = (cnt - lead) >> 1;
            if (t < pairs) *reinterpret_cast<F64x2*>(g + lead + 2 * t) = F64x2{lds_cls[lead + 2 * t], lds_cls[lead + 2 * t + 1]};
            if (t == 0 && lead) g[0] = lds_cls[0];
            if (t == 1 && ((cnt - lead) & 1)) g[cnt - 1] = lds_cls[cnt - 1];
        }
        // (the next pass writes `stage` at once: every lane has read its dwords before the barrier above; it writes the
        // image only behind its own first barrier, which every lane reaches after these stores' LDS reads)
    }
    if (hist) {
        __syncthreads();
        const uint32_t mine = bins[t];
        if (mine) atomicAdd(&hist[t], (unsigned long long)mine);
    }
}

constexpr int kStandardLength[11] = {20, 28, 26, 34, 57, 63, 30, 36, 38, 59, 67};

bool finite3(const double* v) {
    return std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]);
}

}  // namespace

extern "C" int sn_las_chunk_records(void) { return kChunk; }

extern "C" int sn_las_decode(const void* records, int64_t n, int point_format, int record_length, const double scale[3],
                             const double offset[3], double* pts, double* classes, int64_t* hist, sn_stream_t stream) {
    if (!records) return sn::fail(SN_ERR_INVALID_ARG, "sn_las_decode: records is null");
    if (!pts) return sn::fail(SN_ERR_INVALID_ARG, "sn_las_decode: pts is null");
    if (!scale || !offset) return sn::fail(SN_ERR_INVALID_ARG, "sn_las_decode: scale / offset is null");
    if (n <= 0) return sn::fail(SN_ERR_INVALID_ARG, "sn_las_decode: n must be positive (got %lld)", (long long)n);
    if (point_format < 0 || point_format > 10)
        return sn::fail(SN_ERR_INVALID_ARG, "sn_las_decode: point_format must lie in 0..10 (got %d)", point_format);
    if (record_length < kStandardLength[point_format] || record_length > 65535)
        return sn::fail(SN_ERR_INVALID_ARG, "sn_las_decode: record_length %d outside %d..65535 for point format %d",
                        record_length, kStandardLength[point_format], point_format);
    if (!finite3(scale) || !finite3(offset))
        return sn::fail(SN_ERR_INVALID_ARG, "sn_las_decode: scale and offset must be finite");
    if ((uintptr_t)pts % 8 || (uintptr_t)classes % 8 || (uintptr_t)hist % 8)
        return sn::fail(SN_ERR_INVALID_ARG, "sn_las_decode: pts / classes / hist must be 8-byte aligned");
    if (n > kMaxRecords) return sn::fail(SN_ERR_UNSUPPORTED, "sn_las_decode: n > 2^36 records is not served");
    LasShape sh;
    sh.n = n;
    sh.stride = record_length;
    sh.class_byte = point_format >= 6 ? 16 : 15;
    sh.class_mask = point_format >= 6 ? 255u : 31u;
    for (int i = 0; i < 3; ++i) {
        sh.scale[i] = scale[i];
        sh.offset[i] = offset[i];
    }
    const int64_t chunks = (n + kChunk - 1) / kChunk;
    const dim3 grid((unsigned)(chunks < kMaxBlocks ? chunks : kMaxBlocks)), block(kThreads);
    const uint8_t* r = static_cast<const uint8_t*>(records);
    unsigned long long* h = reinterpret_cast<unsigned long long*>(hist);
    hipStream_t s = sn::as_stream(stream);
    if (record_length <= kMaxStagedStride) {
        // granules a chunk's span can take, whatever its alignment, and how many of them a lane carries
        const int granules = (15 + kChunk * record_length + 15) >> 4;
        const int per_lane = (granules + kThreads - 1) / kThreads;   // 2 (20..31 B), 3 (..47), 4 (..63), 5 or 6 (..80)
        const size_t lds = (size_t)per_lane * kThreads * 16;
        if (per_lane <= 2)
            hipLaunchKernelGGL(las_decode_kernel<2>, grid, block, 2 * kThreads * 16, s, r, sh, pts, classes, h);
        else if (per_lane == 3)
            hipLaunchKernelGGL(las_decode_kernel<3>, grid, block, lds, s, r, sh, pts, classes, h);
        else if (per_lane == 4)
            hipLaunchKernelGGL(las_decode_kernel<4>, grid, block, lds, s, r, sh, pts, classes, h);
        else
            hipLaunchKernelGGL(las_decode_kernel<6>, grid, block, 6 * kThreads * 16, s, r, sh, pts, classes, h);
    } else {
        hipLaunchKernelGGL(las_decode_kernel<0>, grid, block, 0, s, r, sh, pts, classes, h);
    }
    return sn::check_launch("sn_las_decode");
}
