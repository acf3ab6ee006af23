// K15 -- LAS encode: pts [n,3] f64, classes [n] f64 and the optional intensity / GPS time / RGB columns -> the point records
// of an uncompressed .las file, with the integer bounding box, the class histogram and the counts of what did not fit
// (sn_las_encode).  The mirror image of K13 (las.hip): the same bytes, moving the other way.
// replaces: what a user of the reference would do to hand a result back in the format it came in -- copy xyz and classes to
//           the host (32 B per point), quantise three fp64 columns with np.rint((x - offset) / scale) (laspy's assignment
//           to a scaled dimension) and pack the unaligned 20..38-byte records into a structured array on one host core.
//           Here the records are quantised and packed where the bandwidth is, and the host writes the bytes as they are.
//
// Definition (normative, include/scenenet_hip.h).  X = rint(fl(fl(x - ox) / sx)): a subtraction and a TRUE fp64 division,
// each rounded once and never contracted (this file is built with -ffp-contract=off), rint to even; NaN -> 0, a quotient
// below -2^31 -> INT32_MIN, above 2^31 - 1 -> INT32_MAX, each counted once per point in bad[0].  The class is written when it
// is an integer of 0..31 (formats 0..3, byte 15, flag bits zero) or 0..255 (formats 6..8, byte 16); otherwise 0 is written
// and bad[1] gains one.  Byte 14 says "return 1 of 1"; every field not named by the interface is 0, and so is every byte
// behind the format's standard length.
//
// Shape.  One workgroup of 256 lanes encodes kChunk = 256 records per pass, one record per lane, and walks the chunks
// c = blockIdx.x, blockIdx.x + gridDim.x, ... (the grid is capped at kMaxBlocks, so the statistics stay on chip over all of
// a workgroup's chunks and are flushed once).  `records` is 16-byte aligned and 256 * record_length is a multiple of 16, so
// every chunk's byte span starts on a granule.  record_length is rarely a multiple of 4, so a lane's record shares its
// first and its last dword with its neighbours': the lane shifts its (at most ten) content dwords by its record's byte
// residue and ORs them into a ZEROED LDS image of the span with ds_or_b32 -- no byte-wide access anywhere, and the bytes
// behind the standard length are zero without being written.  After a barrier lane t reads the image's granules t, t + 256,
// ..., clears them for the next pass and stores them with 16-byte global stores; only the last granule of the last span,
// when n * record_length is no multiple of 16, goes out as an 8-, a 4-, a 2- and a 1-byte store, as its length's bits say.
// The inputs of the NEXT chunk (three doubles of pts and the optional columns) are loaded into registers one pass ahead.
// Per chunk: two barriers.  Box and bad counts live in registers until the workgroup's last chunk, then are reduced through
// LDS atomics; the histogram is summed in LDS per record, as K13's is.
//
// Bound: HBM.  Algorithmic bytes per point: 24 read (+ 8 classes, 2 intensity, 8 GPS time, 6 RGB), record_length written --
// 68 B at format 1 with classes and GPS time.  LDS per point: at most eleven ds_or_b32, record_length read and cleared.
#include "common.h"
#include <cmath>

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kChunk = 256;             // records per workgroup and pass: one per lane
constexpr int kMaxBlocks = 2048;        // 256 CUs x 8 workgroups; further chunks are walked
constexpr int kMaxStride = 80;          // K13's kMaxStagedStride: what the decode stages, the encode serves
constexpr int kContentWords = 10;       // dwords that hold the longest served record's defined fields (format 8: 38 bytes)
constexpr int kSlackBytes = 48;         // a lane ORs dwords 0..kContentWords from the one that holds its byte 0: 44 bytes at most
constexpr int64_t kMaxRecords = (int64_t)1 << 36;             // a workgroup's LDS counters count in 32 bits

typedef uint32_t U32x4 __attribute__((ext_vector_type(4)));   // 16 bytes, 16-byte aligned

struct EncodeShape {
    int64_t n;
    int stride;        // record_length
    int fmt;           // 0, 1, 2, 3, 6, 7 or 8
    int words;         // content dwords of the format: ceil(standard length / 4)
    double class_max;  // 31 | 255
    double scale[3], offset[3];
};

// what a lane holds for one record; loaded one pass ahead
struct Inputs {
    double x, y, z, c;
    uint64_t gps;
    uint32_t intensity, r, g, b;
};

__device__ __forceinline__ void load_inputs(Inputs& in, int64_t i, const double* __restrict__ pts,
                                            const double* __restrict__ classes, const uint16_t* __restrict__ intensity,
                                            const uint64_t* __restrict__ gps, const uint16_t* __restrict__ rgb) {
    in.x = pts[3 * i + 0];
    in.y = pts[3 * i + 1];
    in.z = pts[3 * i + 2];
    in.c = classes ? classes[i] : 0.0;
    in.gps = gps ? gps[i] : 0ull;
    in.intensity = intensity ? (uint32_t)intensity[i] : 0u;
    in.r = rgb ? (uint32_t)rgb[3 * i + 0] : 0u;
    in.g = rgb ? (uint32_t)rgb[3 * i + 1] : 0u;
    in.b = rgb ? (uint32_t)rgb[3 * i + 2] : 0u;
}

// rint(fl(fl(v - o) / s)) saturated to int32; `bad` is set when the quotient is NaN or outside [-2^31, 2^31 - 1]
__device__ __forceinline__ int32_t quantise(double v, double o, double s, bool& bad) {
    const double d = v - o;
    const double q = d / s;
    const bool nan = q != q, low = q < -2147483648.0, high = q > 2147483647.0;
    bad = bad || nan || low || high;
    // (selects, no branches; the conversion of a value outside int32 is never the one selected)
    const int32_t r = (int32_t)__builtin_rint(nan || low || high ? 0.0 : q);
    return nan ? 0 : low ? INT32_MIN : high ? INT32_MAX : r;
}

// Dynamic LDS, all of it (so that its base is 16-byte aligned whatever the compiler does with statics):
//   image  [image_bytes]  the chunk's span as it will lie in memory, plus kSlackBytes, a multiple of 16
//   bins   [256] u32      the workgroup's class histogram
//   sbox   [6]   i32      min X, max X, min Y, max Y, min Z, max Z
//   sbad   [2]   u32
// (8 waves per SIMD: the 2048 workgroups of a full grid are all resident, 8 per CU)
__global__ __launch_bounds__(kThreads, 8) void las_encode_kernel(
    const double* __restrict__ pts, const double* __restrict__ classes, const uint16_t* __restrict__ intensity,
    const uint64_t* __restrict__ gps, const uint16_t* __restrict__ rgb, EncodeShape sh, int image_bytes,
    uint8_t* __restrict__ records, int* __restrict__ box, unsigned long long* __restrict__ hist,
    unsigned long long* __restrict__ bad) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    U32x4* image = reinterpret_cast<U32x4*>(smem);
    uint32_t* image_words = reinterpret_cast<uint32_t*>(smem);
    uint32_t* bins = reinterpret_cast<uint32_t*>(smem + image_bytes);
    int* sbox = reinterpret_cast<int*>(bins + 256);
    uint32_t* sbad = reinterpret_cast<uint32_t*>(sbox + 6);
    const int t = threadIdx.x;
    for (int g = t; g < (image_bytes >> 4); g += kThreads) image[g] = U32x4{0u, 0u, 0u, 0u};
    bins[t] = 0;   // (kThreads == 256)
    if (t < 6) sbox[t] = (t & 1) ? INT32_MIN : INT32_MAX;
    if (t < 2) sbad[t] = 0;
    __syncthreads();   // (the first pass ORs into granules other lanes have cleared)

    const int64_t chunks = (sh.n + kChunk - 1) / kChunk;
    int lo[3] = {INT32_MAX, INT32_MAX, INT32_MAX}, hi[3] = {INT32_MIN, INT32_MIN, INT32_MIN};
    uint32_t bad_xyz = 0, bad_cls = 0;
    Inputs next = {};
    {   // (gridDim.x <= chunks: every workgroup has a first chunk)
        const int64_t i = (int64_t)blockIdx.x * kChunk + t;
        if (i < sh.n) load_inputs(next, i, pts, classes, intensity, gps, rgb);
    }

    for (int64_t c = blockIdx.x; c < chunks; c += gridDim.x) {
        const int64_t first = c * kChunk;
        const int cnt = (int)((sh.n - first) < kChunk ? (sh.n - first) : kChunk);
        const Inputs in = next;
        {
            const int64_t i = (c + gridDim.x) * kChunk + t;
            if (i < sh.n) load_inputs(next, i, pts, classes, intensity, gps, rgb);
        }
        if (t < cnt) {
            bool out_of_range = false;
            const int32_t X = quantise(in.x, sh.offset[0], sh.scale[0], out_of_range);
            const int32_t Y = quantise(in.y, sh.offset[1], sh.scale[1], out_of_range);
            const int32_t Z = quantise(in.z, sh.offset[2], sh.scale[2], out_of_range);
            bad_xyz += out_of_range ? 1u : 0u;
            lo[0] = X < lo[0] ? X : lo[0];
            hi[0] = X > hi[0] ? X : hi[0];
            lo[1] = Y < lo[1] ? Y : lo[1];
            hi[1] = Y > hi[1] ? Y : hi[1];
            lo[2] = Z < lo[2] ? Z : lo[2];
            hi[2] = Z > hi[2] ? Z : hi[2];
            uint32_t cls = 0;
            if (in.c == __builtin_floor(in.c) && in.c >= 0.0 && in.c <= sh.class_max)   // (false for NaN and +-inf)
                cls = (uint32_t)in.c;
            else
                ++bad_cls;
            if (hist) atomicAdd(&bins[cls], 1u);

            // the record's defined bytes as dwords r[0 .. words); r[kContentWords] = 0 closes the shift below
            uint32_t r[kContentWords + 1] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
            r[0] = (uint32_t)X;
            r[1] = (uint32_t)Y;
            r[2] = (uint32_t)Z;
            const uint32_t gl = (uint32_t)in.gps, gh = (uint32_t)(in.gps >> 32);
            if (sh.fmt < 6) {
                r[3] = in.intensity | (0x09u << 16) | (cls << 24);   // bytes 12..15: intensity, return 1 of 1, class
                const uint32_t rg = in.r | (in.g << 16);             // (bytes 16..19: scan angle, user data, source: 0)
                if (sh.fmt & 1) {   // formats 1, 3: GPS time at byte 20, format 3's RGB behind it
                    r[5] = gl;
                    r[6] = gh;
                    if (sh.fmt & 2) {
                        r[7] = rg;
                        r[8] = in.b;
                    }
                } else if (sh.fmt & 2) {   // format 2: RGB at byte 20
                    r[5] = rg;
                    r[6] = in.b;
                }
            } else {
                r[3] = in.intensity | (0x11u << 16);                 // bytes 12..15: intensity, return 1 of 1, flags 0
                r[4] = cls;                                          // bytes 16..19: class, user data 0, scan angle 0
                r[5] = gl << 16;                                     // bytes 20..23: source 0, GPS time bytes 0..1
                r[6] = (gl >> 16) | (gh << 16);                      // GPS time bytes 2..5
                r[7] = (gh >> 16) | (sh.fmt >= 7 ? (in.r << 16) : 0u);   // GPS time bytes 6..7, red
                if (sh.fmt >= 7) r[8] = in.g | (in.b << 16);         // (format 8: NIR at bytes 36..37 is 0, r[9] = 0)
            }
            // the record's byte 0 is byte k of the image's dword o >> 2: dword j from there takes the upper k bytes of
            // r[j - 1] as its lower k bytes and the lower 4 - k bytes of r[j] above them
            const int o = t * sh.stride;
            const uint32_t k = (uint32_t)o & 3u;
            uint32_t* w = image_words + (o >> 2);
            uint32_t prev = 0;
#pragma unroll
            for (int j = 0; j <= kContentWords; ++j) {
                if (j <= sh.words) {   // (uniform; index (o >> 2) + j <= (255 * 80 + 44) / 4: inside the slack)
                    const uint32_t v = k ? __builtin_amdgcn_alignbyte(r[j], prev, 4u - k) : r[j];
                    atomicOr(&w[j], v);   // (ds_or_b32 without a return value)
                    prev = r[j];
                }
            }
        }
        __syncthreads();
        // the image goes out: bytes [0, cnt * stride) to records + first * stride, whole granules with 16-byte stores; every
        // granule read is cleared for the next pass by the lane that read it
        {
            uint8_t* span = records + first * (int64_t)sh.stride;   // 64-bit: n * record_length may pass 2^31
            const int bytes = cnt * sh.stride;
            const int whole = bytes >> 4;
            const int granules = (bytes + kSlackBytes + 15) >> 4;   // (what the ORs may have touched; <= image_bytes / 16)
            for (int g = t; g < granules; g += kThreads) {
                const U32x4 v = image[g];
                image[g] = U32x4{0u, 0u, 0u, 0u};
                if (g < whole) {
                    reinterpret_cast<U32x4*>(span)[g] = v;
                } else if (g == whole) {
                    // the last span's tail of bytes & 15 bytes (0 for every span but the file's last): 8, 4, 2, 1
                    uint8_t* p = span + ((int64_t)whole << 4);
                    int at = 0;
                    if (bytes & 8) {
                        *reinterpret_cast<uint2*>(p) = make_uint2(v[0], v[1]);
                        at = 2;
                    }
                    if (bytes & 4) {
                        *reinterpret_cast<uint32_t*>(p + 4 * at) = at ? v[2] : v[0];
                        ++at;
                    }
                    if (bytes & 3) {
                        const uint32_t last = at == 0 ? v[0] : at == 1 ? v[1] : at == 2 ? v[2] : v[3];
                        uint8_t* q = p + 4 * at;
                        if (bytes & 2) *reinterpret_cast<uint16_t*>(q) = (uint16_t)last;
                        if (bytes & 1) q[bytes & 2] = (uint8_t)(last >> ((bytes & 2) * 8));
                    }
                }
            }
        }
        __syncthreads();   // (the next pass ORs into granules other lanes have just cleared)
    }

    // the workgroup's statistics, once
    if (box) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            if (lo[a] <= hi[a]) {   // (a lane that has seen a record)
                atomicMin(&sbox[2 * a], lo[a]);
                atomicMax(&sbox[2 * a + 1], hi[a]);
            }
        }
    }
    if (bad) {
        if (bad_xyz) atomicAdd(&sbad[0], bad_xyz);
        if (bad_cls) atomicAdd(&sbad[1], bad_cls);
    }
    __syncthreads();
    if (hist) {
        const uint32_t mine = bins[t];
        if (mine) atomicAdd(&hist[t], (unsigned long long)mine);
    }
    if (box && t < 6) {   // (every workgroup has encoded a record: its box is a true one)
        if (t & 1)
            atomicMax(&box[t], sbox[t]);
        else
            atomicMin(&box[t], sbox[t]);
    }
    if (bad && t < 2 && sbad[t]) atomicAdd(&bad[t], (unsigned long long)sbad[t]);
}

constexpr int kStandardLength[11] = {20, 28, 26, 34, 57, 63, 30, 36, 38, 59, 67};

bool finite3(const double* v) {
    return std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]);
}

}  // namespace

extern "C" int sn_las_encode_chunk_records(void) { return kChunk; }

extern "C" int sn_las_encode(const double* pts, const double* classes, const uint16_t* intensity, const double* gps_time,
                             const uint16_t* rgb, int64_t n, int point_format, int record_length, const double scale[3],
                             const double offset[3], void* records, int32_t* box, int64_t* hist, int64_t* bad,
                             sn_stream_t stream) {
    if (!pts) return sn::fail(SN_ERR_INVALID_ARG, "sn_las_encode: pts is null");
    if (!records) return sn::fail(SN_ERR_INVALID_ARG, "sn_las_encode: records is null");
    if (!scale || !offset) return sn::fail(SN_ERR_INVALID_ARG, "sn_las_encode: scale / offset is null");
    if (n <= 0) return sn::fail(SN_ERR_INVALID_ARG, "sn_las_encode: n must be positive (got %lld)", (long long)n);
    if (point_format < 0 || point_format > 10)
        return sn::fail(SN_ERR_INVALID_ARG, "sn_las_encode: point_format must lie in 0..10 (got %d)", point_format);
    if (record_length < kStandardLength[point_format])
        return sn::fail(SN_ERR_INVALID_ARG, "sn_las_encode: record_length %d is below the %d bytes of point format %d",
                        record_length, kStandardLength[point_format], point_format);
    if (!finite3(scale) || scale[0] == 0.0 || scale[1] == 0.0 || scale[2] == 0.0)
        return sn::fail(SN_ERR_INVALID_ARG, "sn_las_encode: scale must be finite and not zero");
    if (!finite3(offset)) return sn::fail(SN_ERR_INVALID_ARG, "sn_las_encode: offset must be finite");
    const bool has_gps = point_format == 1 || point_format == 3 || point_format >= 6;
    const bool has_rgb = point_format == 2 || point_format == 3 || point_format == 5 || point_format == 7 ||
                         point_format == 8 || point_format == 10;
    if (gps_time && !has_gps)
        return sn::fail(SN_ERR_INVALID_ARG, "sn_las_encode: point format %d holds no gps_time", point_format);
    if (rgb && !has_rgb) return sn::fail(SN_ERR_INVALID_ARG, "sn_las_encode: point format %d holds no rgb", point_format);
    if ((uintptr_t)records % 16)
        return sn::fail(SN_ERR_INVALID_ARG, "sn_las_encode: records must be 16-byte aligned");
    if ((uintptr_t)pts % 8 || (uintptr_t)classes % 8 || (uintptr_t)gps_time % 8 || (uintptr_t)hist % 8 || (uintptr_t)bad % 8 ||
        (uintptr_t)box % 4 || (uintptr_t)intensity % 2 || (uintptr_t)rgb % 2)
        return sn::fail(SN_ERR_INVALID_ARG, "sn_las_encode: pts / classes / gps_time / hist / bad must be 8-byte aligned, box "
                                            "4-byte, intensity / rgb 2-byte");
    if (point_format == 4 || point_format == 5 || point_format == 9 || point_format == 10)
        return sn::fail(SN_ERR_UNSUPPORTED, "sn_las_encode: the waveform point format %d is not served", point_format);
    if (record_length > kMaxStride)
        return sn::fail(SN_ERR_UNSUPPORTED, "sn_las_encode: record_length %d above %d is not served", record_length, kMaxStride);
    if (n > kMaxRecords) return sn::fail(SN_ERR_UNSUPPORTED, "sn_las_encode: n > 2^36 records is not served");
    EncodeShape sh;
    sh.n = n;
    sh.stride = record_length;
    sh.fmt = point_format;
    sh.words = (kStandardLength[point_format] + 3) / 4;
    sh.class_max = point_format >= 6 ? 255.0 : 31.0;
    for (int i = 0; i < 3; ++i) {
        sh.scale[i] = scale[i];
        sh.offset[i] = offset[i];
    }
    const int64_t chunks = (n + kChunk - 1) / kChunk;
    const dim3 grid((unsigned)(chunks < kMaxBlocks ? chunks : kMaxBlocks)), block(kThreads);
    const int image_bytes = (kChunk * record_length + kSlackBytes + 15) & ~15;
    const size_t lds = (size_t)image_bytes + 256 * 4 + 6 * 4 + 2 * 4;   // at most 21600 bytes: no attribute to raise
    hipLaunchKernelGGL(las_encode_kernel, grid, block, lds, sn::as_stream(stream), pts, classes, intensity,
                       reinterpret_cast<const uint64_t*>(gps_time), rgb, sh, image_bytes, static_cast<uint8_t*>(records),
                       reinterpret_cast<int*>(box), reinterpret_cast<unsigned long long*>(hist),
                       reinterpret_cast<unsigned long long*>(bad));
    return sn::check_launch("sn_las_encode");
}
