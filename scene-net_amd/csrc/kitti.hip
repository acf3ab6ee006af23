// K14 -- SemanticKITTI decode: the velodyne (.bin) and label (.label) bytes of B scans -> pts [total,3] f64, labels
// [total] f64, remission, instance ids and a per-scan class census (sn_kitti_decode).
// replaces: core/datasets/semKITTI.py:388-403 -- SemLaserScan.open_scan / open_label (np.fromfile, reshape((-1, 4)),
//           `label & 0xFFFF`, `label >> 16`) per scan on one host core, the widening to fp64 and an upload per scan.  Here the
//           bytes of a batch of scans travel host-to-device as the files hold them and are decoded in one launch.
// Provenance: the reference imports SemKITTI_API.auxiliary.laserscan.SemLaserScan (semKITTI.py:26), which it does not
//           carry, so nothing here is pinned against the reference's own output.  The layout is the published
//           SemanticKITTI one: .bin is little-endian float32 [n,4] (x, y, z, remission), .label little-endian uint32 [n],
//           semantic class in the low 16 bits, instance id in the high 16.
//
// Definition (normative, include/scenenet_hip.h).  pts = the exact widening of x, y, z, by integer arithmetic, the rule of
// sn_tiles_unpack's f32 rows; remission = the bits of column 3; sem = w & 0xFFFF, instance = w >> 16; the output class c is
// sem, or lut[sem] (-1 and one more in unmapped[b] where sem >= n_lut); labels = (double)c; hist[b][c] gains one where
// 0 <= c < n_hist; bad[b] counts the points of scan b with a non-finite x, y or z.
//
// Shape.  One workgroup of 256 lanes decodes kChunk = 256 points per pass, one point per lane.  The grid is capped at
// kMaxBlocks workgroups; each takes a CONTIGUOUS run of chunks (not a grid stride), so that the scan its census belongs to
// changes only where a scan really ends: the census of the current scan lives in LDS (n_hist bins and the two counters) and
// is added to memory -- 64-bit integer atomics, non-zero bins only -- when the run crosses into another scan and at the
// end.  The scan of a pass's first point is found by one workgroup-uniform binary search of `offsets`; from there the pass
// is walked segment by segment (a segment: the part of the chunk that lies in one scan), uniformly, so no lane searches.
// A point is one 16-byte load when `scans` is 16-byte aligned, four dwords otherwise.  The chunk's label words are loaded
// as the aligned 16-byte granules that hold them (at most 65, one per lane) and read from LDS.  Both loads are issued ONE
// PASS AHEAD into registers, so they are in flight while the current pass decodes and stores.  pts and labels
// are left in LDS as they will lie in memory and stored as las.hip stores its image: 16 bytes per lane, an 8-byte store at
// either end where the chunk's part starts or ends on an odd multiple of 8.  remission and instance are one dword per lane.
//
// Bound: HBM.  Algorithmic bytes per point: 16 + 4 read, 24 + 8 written (52), + 4 with remission, + 4 with instance.
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kChunk = 256;             // points per workgroup and pass: one per lane
constexpr int kMaxBlocks = 2048;        // 256 CUs x 8 workgroups; beyond, a workgroup takes several consecutive chunks
constexpr int kMaxHist = 1024;
constexpr int kMaxLut = 65536;
constexpr int64_t kMaxTotal = (int64_t)1 << 36;   // a workgroup's LDS census counts in 32 bits: 2^36 / kMaxBlocks points
constexpr int kMaxScans = 1 << 20;

typedef uint32_t U32x4 __attribute__((ext_vector_type(4)));   // 16 bytes, 16-byte aligned
typedef double F64x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ bool nonfinite32(uint32_t u) { return (u & 0x7f800000u) == 0x7f800000u; }

struct KittiArgs {
    const uint32_t* scans;      // [total,4]
    const uint32_t* words;      // [total] | null
    const int64_t* offsets;     // [B+1]
    const int32_t* lut;         // [n_lut] | null
    uint64_t* pts;              // [total,3]
    uint64_t* labels;           // [total] | null
    uint32_t* remission;        // [total] | null
    int32_t* instance;          // [total] | null
    unsigned long long* hist;   // [B,n_hist] | null
    int32_t* bad;               // [B] | null
    int32_t* unmapped;          // [B] | null
    int64_t total, chunks;
    int B, n_lut, n_hist;
};

// the census of scan b as the workgroup holds it -> memory, and the LDS copy cleared.  Every lane of the workgroup calls.
__device__ __forceinline__ void flush_census(const KittiArgs& a, int b, uint32_t* bins, uint32_t* counters, int t) {
    __syncthreads();   // (every add of the passes so far has landed)
    if (a.hist) {
        for (int c = t; c < a.n_hist; c += kThreads) {
            const uint32_t v = bins[c];
            if (v) {
                atomicAdd(&a.hist[(int64_t)b * a.n_hist + c], (unsigned long long)v);
                bins[c] = 0;
            }
        }
    }
    if (t < 2) {
        const uint32_t v = counters[t];
        int32_t* dst = t == 0 ? a.bad : a.unmapped;
        if (v && dst) atomicAdd(&dst[b], (int32_t)v);
        counters[t] = 0;
    }
    __syncthreads();   // (cleared before the next add)
}

// what a lane keeps in registers for the NEXT pass: its point's row and one granule of the chunk's label words.  A granule's
// bytes in front of the first word or behind the last one are READ only when the granule holds a word of the chunk (an
// aligned 16-byte granule lies in one page, the page of that word), and are never used.
template <bool kAligned>
struct Prefetch {
    U32x4 row, granule;
    int head;   // words between the granule-aligned address and the chunk's first word (0..3)
    __device__ __forceinline__ void issue(const KittiArgs& a, int64_t c, int t) {
        const int64_t first = c * kChunk;
        const int cnt = (int)((a.total - first) < kChunk ? (a.total - first) : kChunk);
        row = U32x4{0u, 0u, 0u, 0u};
        if (t < cnt) {
            if (kAligned) {
                row = *reinterpret_cast<const U32x4*>(a.scans + (first + t) * 4);
            } else {
                const uint32_t* r = a.scans + (first + t) * 4;
                row = U32x4{r[0], r[1], r[2], r[3]};
            }
        }
        head = 0;
        granule = U32x4{0u, 0u, 0u, 0u};
        if (a.words) {
            const uint32_t* w0 = a.words + first;
            head = (int)((reinterpret_cast<uintptr_t>(w0) >> 2) & 3);
            const int granules = (head + cnt + 3) >> 2;   // <= kChunk / 4 + 1
            if (t < granules) granule = reinterpret_cast<const U32x4*>(w0 - head)[t];
        }
    }
};

template <bool kAligned>   // scans 16-byte aligned: one 16-byte load per point
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(8, 8)))
void kitti_decode_kernel(KittiArgs a) {
    __shared__ F64x2 out_pts[kChunk * 3 / 2];
    __shared__ F64x2 out_lab[kChunk / 2];
    __shared__ U32x4 stage[kChunk / 4 + 1];   // the chunk's label words, from the aligned granule of the first one
    __shared__ uint32_t bins[kMaxHist];
    __shared__ uint32_t counters[2];          // bad, unmapped of the current scan
    const int t = threadIdx.x;
    const bool census = a.hist || a.bad || a.unmapped;
    if (census) {
        for (int c = t; c < kMaxHist; c += kThreads) bins[c] = 0;
        if (t < 2) counters[t] = 0;
    }
    uint64_t* lds_pts = reinterpret_cast<uint64_t*>(out_pts);
    uint64_t* lds_lab = reinterpret_cast<uint64_t*>(out_lab);
    const uint32_t* stage_words = reinterpret_cast<const uint32_t*>(stage);
    // this workgroup's run of chunks: an even split (gridDim.x <= chunks, so every workgroup has one at least)
    const int64_t c0 = (int64_t)blockIdx.x * a.chunks / gridDim.x;
    const int64_t c1 = ((int64_t)blockIdx.x + 1) * a.chunks / gridDim.x;
    int cur = -1;   // the scan whose census the LDS holds (workgroup-uniform)
    Prefetch<kAligned> pre;
    pre.issue(a, c0, t);

    for (int64_t c = c0; c < c1; ++c) {
        const int64_t first = c * kChunk;
        const int cnt = (int)((a.total - first) < kChunk ? (a.total - first) : kChunk);
        const int64_t i = first + t;
        // this pass's loads wait in registers since the previous pass; while the lanes decode and store, the next pass's
        // are in flight
        const U32x4 row = pre.row;
        const int head = pre.head;
        if (a.words && t < kChunk / 4 + 1) stage[t] = pre.granule;
        __syncthreads();   // the words are staged; the previous pass's image has been stored by every lane
        if (c + 1 < c1) pre.issue(a, c + 1, t);

        int32_t cls = 0;
        bool is_bad = false, is_unmapped = false;
        if (t < cnt) {
            lds_pts[3 * t + 0] = sn::widen_f32_bits(row.x);
            lds_pts[3 * t + 1] = sn::widen_f32_bits(row.y);
            lds_pts[3 * t + 2] = sn::widen_f32_bits(row.z);
            is_bad = nonfinite32(row.x) || nonfinite32(row.y) || nonfinite32(row.z);
            if (a.remission) a.remission[i] = row.w;
            if (a.words) {
                const uint32_t w = stage_words[head + t];
                const uint32_t sem = w & 0xffffu;
                cls = (int32_t)sem;
                if (a.lut) {
                    is_unmapped = sem >= (uint32_t)a.n_lut;
                    cls = is_unmapped ? -1 : a.lut[sem];
                }
                lds_lab[t] = (uint64_t)__double_as_longlong((double)cls);
                if (a.instance) a.instance[i] = (int32_t)(w >> 16);
            }
        }

        if (census) {
            // the scan of the pass's first point: the last b with offsets[b] <= first, inside [0, B) whatever offsets holds
            int b;
            if (cur >= 0 && (cur + 1 >= a.B || a.offsets[cur + 1] > first)) {
                b = cur;   // (the run is still inside the scan of the previous pass)
            } else {
                int lo = 0, hi = a.B;
                while (hi - lo > 1) {
                    const int mid = lo + ((hi - lo) >> 1);
                    if (a.offsets[mid] <= first) lo = mid; else hi = mid;
                }
                b = lo;
            }
            // segments: [seg, end) lies in scan b.  Every quantity is workgroup-uniform; each turn moves seg forward.
            const int64_t stop = first + cnt;
            int64_t seg = first;
            while (seg < stop) {
                while (b + 1 < a.B && a.offsets[b + 1] <= seg) ++b;   // (steps over empty scans)
                int64_t end = stop;
                if (b + 1 < a.B && a.offsets[b + 1] < end) end = a.offsets[b + 1];   // (> seg by the loop above)
                if (b != cur) {
                    if (cur >= 0) flush_census(a, cur, bins, counters, t);
                    cur = b;
                }
                const bool mine = i >= seg && i < end;
                if (a.hist && mine && cls >= 0 && cls < a.n_hist) atomicAdd(&bins[cls], 1u);
                const unsigned long long nb = __ballot(mine && is_bad), nu = __ballot(mine && is_unmapped);
                if ((t & 63) == 0) {
                    if (nb) atomicAdd(&counters[0], (uint32_t)__popcll(nb));
                    if (nu) atomicAdd(&counters[1], (uint32_t)__popcll(nu));
                }
                seg = end;
            }
        }
        __syncthreads();
        // the chunk's image: 3 * cnt doubles of pts from pts + 3 * first, cnt doubles of labels from labels + first; a lane
        // stores pairs that are 16-byte aligned in MEMORY, lanes 0 and 1 the single doubles at the two ends
        {
            uint64_t* g = a.pts + 3 * first;
            const int m = 3 * cnt;
            const int lead = (int)((reinterpret_cast<uintptr_t>(g) >> 3) & 1);   // (m >= 3 > lead)
            const int pairs = (m - lead) >> 1;
            for (int j = t; j < pairs; j += kThreads) {
                const F64x2 v = {__longlong_as_double((long long)lds_pts[lead + 2 * j]),
                                 __longlong_as_double((long long)lds_pts[lead + 2 * j + 1])};
                *reinterpret_cast<F64x2*>(g + lead + 2 * j) = v;
            }
            if (t == 0 && lead) g[0] = lds_pts[0];
            if (t == 1 && ((m - lead) & 1)) g[m - 1] = lds_pts[m - 1];
        }
        if (a.labels) {
            uint64_t* g = a.labels + first;
            const int lead = (int)((reinterpret_cast<uintptr_t>(g) >> 3) & 1);   // cnt == 1 with lead: no pair, no tail
            const int pairs = (cnt - lead) >> 1;
            if (t < pairs) {
                const F64x2 v = {__longlong_as_double((long long)lds_lab[lead + 2 * t]),
                                 __longlong_as_double((long long)lds_lab[lead + 2 * t + 1])};
                *reinterpret_cast<F64x2*>(g + lead + 2 * t) = v;
            }
            if (t == 0 && lead) g[0] = lds_lab[0];
            if (t == 1 && ((cnt - lead) & 1)) g[cnt - 1] = lds_lab[cnt - 1];
        }
        // (the next pass writes `stage` at once: every lane read its word before the barrier above; it writes the image
        // only behind its own first barrier, which every lane reaches after these stores' LDS reads)
    }
    if (census && cur >= 0) flush_census(a, cur, bins, counters, t);
}

}  // namespace

extern "C" int sn_kitti_chunk_points(void) { return kChunk; }

extern "C" int sn_kitti_decode(const void* scans, const void* label_words, int64_t total, const int64_t* offsets, int B,
                               const int32_t* lut, int n_lut, double* pts, double* labels, float* remission,
                               int32_t* instance, int64_t* hist, int n_hist, int32_t* bad, int32_t* unmapped,
                               sn_stream_t stream) {
    if (!scans) return sn::fail(SN_ERR_INVALID_ARG, "sn_kitti_decode: scans is null");
    if (!pts) return sn::fail(SN_ERR_INVALID_ARG, "sn_kitti_decode: pts is null");
    if (!offsets) return sn::fail(SN_ERR_INVALID_ARG, "sn_kitti_decode: offsets is null");
    if (total <= 0) return sn::fail(SN_ERR_INVALID_ARG, "sn_kitti_decode: total must be positive (got %lld)", (long long)total);
    if (B <= 0) return sn::fail(SN_ERR_INVALID_ARG, "sn_kitti_decode: B must be positive (got %d)", B);
    if (labels && !label_words) return sn::fail(SN_ERR_INVALID_ARG, "sn_kitti_decode: labels need label_words");
    if (label_words && !labels) return sn::fail(SN_ERR_INVALID_ARG, "sn_kitti_decode: label_words need labels");
    if (instance && !label_words) return sn::fail(SN_ERR_INVALID_ARG, "sn_kitti_decode: instance needs label_words");
    if (lut && !label_words) return sn::fail(SN_ERR_INVALID_ARG, "sn_kitti_decode: lut needs label_words");
    if (hist && !label_words) return sn::fail(SN_ERR_INVALID_ARG, "sn_kitti_decode: hist needs label_words");
    if (lut && (n_lut < 1 || n_lut > kMaxLut))
        return sn::fail(SN_ERR_INVALID_ARG, "sn_kitti_decode: n_lut must lie in 1..%d (got %d)", kMaxLut, n_lut);
    if (hist && (n_hist < 1 || n_hist > kMaxHist))
        return sn::fail(SN_ERR_INVALID_ARG, "sn_kitti_decode: n_hist must lie in 1..%d (got %d)", kMaxHist, n_hist);
    if (unmapped && !lut) return sn::fail(SN_ERR_INVALID_ARG, "sn_kitti_decode: unmapped needs lut");
    if ((uintptr_t)scans % 4 || (uintptr_t)label_words % 4 || (uintptr_t)lut % 4 || (uintptr_t)remission % 4 ||
        (uintptr_t)instance % 4 || (uintptr_t)bad % 4 || (uintptr_t)unmapped % 4)
        return sn::fail(SN_ERR_INVALID_ARG,
                        "sn_kitti_decode: scans / label_words / lut / remission / instance / bad / unmapped must be 4-byte aligned");
    if ((uintptr_t)pts % 8 || (uintptr_t)labels % 8 || (uintptr_t)hist % 8 || (uintptr_t)offsets % 8)
        return sn::fail(SN_ERR_INVALID_ARG, "sn_kitti_decode: pts / labels / hist / offsets must be 8-byte aligned");
    if (total > kMaxTotal) return sn::fail(SN_ERR_UNSUPPORTED, "sn_kitti_decode: total > 2^36 points is not served");
    if (B > kMaxScans) return sn::fail(SN_ERR_UNSUPPORTED, "sn_kitti_decode: B > 2^20 scans is not served");
    hipStream_t s = sn::as_stream(stream);
    if (bad) {
        const hipError_t e = hipMemsetAsync(bad, 0, (size_t)B * sizeof(int32_t), s);
        if (e != hipSuccess) return sn::fail(SN_ERR_LAUNCH, "sn_kitti_decode(clear bad): %s", hipGetErrorString(e));
    }
    if (unmapped) {
        const hipError_t e = hipMemsetAsync(unmapped, 0, (size_t)B * sizeof(int32_t), s);
        if (e != hipSuccess) return sn::fail(SN_ERR_LAUNCH, "sn_kitti_decode(clear unmapped): %s", hipGetErrorString(e));
    }
    KittiArgs a;
    a.scans = static_cast<const uint32_t*>(scans);
    a.words = static_cast<const uint32_t*>(label_words);
    a.offsets = offsets;
    a.lut = lut;
    a.pts = reinterpret_cast<uint64_t*>(pts);
    a.labels = reinterpret_cast<uint64_t*>(labels);
    a.remission = reinterpret_cast<uint32_t*>(remission);
    a.instance = instance;
    a.hist = reinterpret_cast<unsigned long long*>(hist);
    a.bad = bad;
    a.unmapped = unmapped;
    a.total = total;
    a.chunks = (total + kChunk - 1) / kChunk;
    a.B = B;
    a.n_lut = lut ? n_lut : 0;
    a.n_hist = hist ? n_hist : 0;
    const dim3 grid((unsigned)(a.chunks < kMaxBlocks ? a.chunks : kMaxBlocks)), block(kThreads);
    if ((uintptr_t)scans % 16 == 0)
        hipLaunchKernelGGL(kitti_decode_kernel<true>, grid, block, 0, s, a);
    else
        hipLaunchKernelGGL(kitti_decode_kernel<false>, grid, block, 0, s, a);
    return sn::check_launch("sn_kitti_decode");
}
