// K6 -- training metrics of the reference's MetricCollection (utils/scripts_utils.py:80-91: JaccardIndex(num_classes=2),
// Precision, Recall, F1Score, FBetaScore(beta=0.5), all at threshold tau) from the four confusion counts of a binary
// prediction.  One streaming pass counts, per workgroup, (tp, predicted positives, target positives, bad preds, bad
// targets); a one-workgroup kernel sums the partial records in a fixed order, adds them to the caller's running state and
// turns counts into values.  Integer counts: exact and independent of order, no atomics.
//
// Bound: HBM.  Algorithmic bytes per element: sizeof(pred) + sizeof(target), read once.
// Below it, sn_binary_curve: the same counts at T thresholds from one pass (a histogram over the thresholds cleared).
#include "common.h"
#include <type_traits>

namespace {

constexpr int kThreads = 256;
constexpr int kElems = 8;                       // elements per lane per chunk: 16-byte loads of every dtype but u8 (8 bytes)
constexpr int kChunk = kThreads * kElems;       // elements per workgroup per chunk
constexpr int kCombineThreads = 256;
constexpr int64_t kMaxN = (int64_t)1 << 40;     // keeps every per-lane and per-wave u32 counter far from wrapping

using bf16 = __bf16;

template <typename T>
struct Chunk {
    T v[kElems];
};

template <typename T>
constexpr int vec_align() { return kElems * sizeof(T) < 16 ? kElems * sizeof(T) : 16; }

template <typename T>
__device__ __forceinline__ Chunk<T> load_chunk(const T* p) {
    Chunk<T> r;
    if constexpr (kElems * sizeof(T) == 8) {
        const uint2 u = *reinterpret_cast<const uint2*>(p);
        __builtin_memcpy(&r, &u, 8);
    } else {
#pragma unroll
        for (int k = 0; k < (int)(kElems * sizeof(T)) / 16; ++k) {
            const uint4 u = reinterpret_cast<const uint4*>(p)[k];
            __builtin_memcpy(reinterpret_cast<char*>(&r) + 16 * k, &u, 16);
        }
    }
    return r;
}

// pred >= tau in pred's own dtype (tau arrives rounded to it; bf16 widens to fp32 exactly); NaN compares false
template <typename PT> struct PredOf { using type = PT; };
template <> struct PredOf<bf16> { using type = float; };

// int(target) == 1 under C truncation, and "truncation is neither 0 nor 1" (NaN and +-Inf included)
template <typename T>
__device__ __forceinline__ void classify_target(T t, bool& pos, bool& bad) {
    if constexpr (sizeof(T) == 1) {
        pos = t == 1;
        bad = t > 1;
    } else if constexpr (std::is_same<T, int32_t>::value) {
        pos = t == 1;
        bad = (uint32_t)t > 1u;
    } else {
        using C = typename PredOf<T>::type;
        const C c = (C)t;
        pos = c >= (C)1 && c < (C)2;
        bad = !(c > (C)-1 && c < (C)2);
    }
}

struct Counts {
    uint32_t npred, ntgt, tp, bad_pred, bad_tgt;
};

template <typename PT, typename TT>
__device__ __forceinline__ void count_one(PT pv, TT tv, typename PredOf<PT>::type tau, Counts& c) {
    using C = typename PredOf<PT>::type;
    const C p = (C)pv;
    const bool pp = p >= tau;
    bool tt, bt;
    classify_target(tv, tt, bt);
    c.npred += pp;
    c.ntgt += tt;
    c.tp += pp && tt;
    c.bad_pred += (p < (C)0) || (p > (C)1);
    c.bad_tgt += bt;
}

// Partial record of workgroup w: parts[w * SN_METRIC_NCOUNT + {0..4}] = tp, npred, ntgt, bad_pred, bad_tgt (slot 5 unused).
// Elements [0, head) and [head + nvec * kElems, n) go one per thread; the middle goes in chunks whose loads are aligned
// for both operands (head == n when no such split exists: the two pointers are misaligned against each other).
template <typename PT, typename TT>
__global__ __launch_bounds__(kThreads) void metrics_stats_kernel(const PT* __restrict__ pred, const TT* __restrict__ tgt,
                                                                 int64_t n, int64_t head, int64_t nvec,
                                                                 typename PredOf<PT>::type tau,
                                                                 uint64_t* __restrict__ parts) {
    Counts c{0, 0, 0, 0, 0};
    const int tid = threadIdx.x;
    const int64_t gtid = (int64_t)blockIdx.x * kThreads + tid, gstride = (int64_t)gridDim.x * kThreads;
    const PT* p = pred + head;
    const TT* t = tgt + head;
    // two chunks in flight per lane, then one
    int64_t v = (int64_t)blockIdx.x * kThreads + tid;
    for (; v + gstride < nvec; v += 2 * gstride) {
        const Chunk<PT> pa = load_chunk(p + v * kElems), pb = load_chunk(p + (v + gstride) * kElems);
        const Chunk<TT> ta = load_chunk(t + v * kElems), tb = load_chunk(t + (v + gstride) * kElems);
#pragma unroll
        for (int j = 0; j < kElems; ++j) count_one<PT, TT>(pa.v[j], ta.v[j], tau, c);
#pragma unroll
        for (int j = 0; j < kElems; ++j) count_one<PT, TT>(pb.v[j], tb.v[j], tau, c);
    }
    if (v < nvec) {
        const Chunk<PT> pa = load_chunk(p + v * kElems);
        const Chunk<TT> ta = load_chunk(t + v * kElems);
#pragma unroll
        for (int j = 0; j < kElems; ++j) count_one<PT, TT>(pa.v[j], ta.v[j], tau, c);
    }
    for (int64_t i = gtid; i < head; i += gstride) count_one<PT, TT>(pred[i], tgt[i], tau, c);
    for (int64_t i = head + nvec * kElems + gtid; i < n; i += gstride) count_one<PT, TT>(pred[i], tgt[i], tau, c);

    // wave sums (u32: at most 64 lanes x n / 2^18 per lane), then the four waves in LDS as u64
    uint32_t w[5] = {c.tp, c.npred, c.ntgt, c.bad_pred, c.bad_tgt};
#pragma unroll
    for (int k = 0; k < 5; ++k)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) w[k] += __shfl_xor(w[k], off, 64);
    __shared__ uint64_t sh[kThreads / 64][5];
    const int wave = tid >> 6, lane = tid & 63;
    if (lane == 0)
#pragma unroll
        for (int k = 0; k < 5; ++k) sh[wave][k] = w[k];
    __syncthreads();
    if (tid < SN_METRIC_NCOUNT) {
        uint64_t s = 0;
        if (tid < 5)
            for (int q = 0; q < kThreads / 64; ++q) s += sh[q][tid];
        parts[(size_t)blockIdx.x * SN_METRIC_NCOUNT + tid] = s;
    }
}

__device__ __forceinline__ double ratio(double a, double b) { return b == 0.0 ? 0.0 : a / b; }

// JaccardIndex (2-class macro mean), Precision, Recall, F1Score, FBetaScore from (tp, fp, fn, tn) in fp64, 0/0 -> 0.
// metrics.py: binary_metric_values is the same arithmetic, operation for operation (built with -ffp-contract=off).
__device__ void metric_values(const uint64_t* cnt, double beta, float* out) {
    const double tp = (double)cnt[0], fp = (double)cnt[1], fn = (double)cnt[2], tn = (double)cnt[3];
    const double P = ratio(tp, tp + fp), R = ratio(tp, tp + fn);
    const double F1 = ratio(2.0 * P * R, P + R);
    const double b2 = beta * beta;
    const double FB = ratio((1.0 + b2) * P * R, b2 * P + R);
    const double J = 0.5 * (ratio(tp, tp + fp + fn) + ratio(tn, tn + fp + fn));
    out[0] = (float)J;
    out[1] = (float)P;
    out[2] = (float)R;
    out[3] = (float)F1;
    out[4] = (float)FB;
}

__global__ __launch_bounds__(kCombineThreads) void metrics_combine_kernel(const uint64_t* __restrict__ parts, int nparts,
                                                                         int64_t n, double beta,
                                                                         uint64_t* __restrict__ state,
                                                                         uint64_t* __restrict__ batch,
                                                                         float* __restrict__ values) {
    __shared__ uint64_t sh[5][kCombineThreads];
    const int tid = threadIdx.x;
    uint64_t s[5] = {0, 0, 0, 0, 0};
    for (int i = tid; i < nparts; i += kCombineThreads)
#pragma unroll
        for (int k = 0; k < 5; ++k) s[k] += parts[(size_t)i * SN_METRIC_NCOUNT + k];
#pragma unroll
    for (int k = 0; k < 5; ++k) sh[k][tid] = s[k];
    __syncthreads();
    for (int h = kCombineThreads / 2; h > 0; h >>= 1) {
        if (tid < h)
#pragma unroll
            for (int k = 0; k < 5; ++k) sh[k][tid] += sh[k][tid + h];
        __syncthreads();
    }
    if (tid != 0) return;
    const uint64_t tp = sh[0][0], npred = sh[1][0], ntgt = sh[2][0];
    const uint64_t b[SN_METRIC_NCOUNT] = {tp, npred - tp, ntgt - tp, (uint64_t)n - npred - ntgt + tp, sh[3][0], sh[4][0]};
    uint64_t acc[SN_METRIC_NCOUNT];
#pragma unroll
    for (int k = 0; k < SN_METRIC_NCOUNT; ++k) acc[k] = state[k] + b[k];
#pragma unroll
    for (int k = 0; k < SN_METRIC_NCOUNT; ++k) state[k] = acc[k];
    if (batch)
#pragma unroll
        for (int k = 0; k < SN_METRIC_NCOUNT; ++k) batch[k] = b[k];
    if (values) {
        metric_values(b, beta, values);
        metric_values(acc, beta, values + SN_METRIC_NVALUE);
    }
}

int dtype_error(const char* what, int dt) {
    // a known dtype in a role this entry does not take: unsupported; anything else: not a dtype at all
    return sn::fail(dt >= SN_F32 && dt <= SN_I32 ? SN_ERR_UNSUPPORTED : SN_ERR_INVALID_ARG,
                    "sn_binary_stats: %s dtype %d not accepted (pred: SN_F32 | SN_BF16 | SN_F64; target: SN_F32 | SN_F64 | "
                    "SN_BF16 | SN_U8 | SN_OCC8 | SN_I32)", what, dt);
}

// tau rounded to bf16 the way torch rounds a Python scalar for a bf16 comparison: to fp32, then to nearest even
float round_bf16(double tau) {
    const float f = (float)tau;
    uint32_t u;
    __builtin_memcpy(&u, &f, 4);
    u = (u + 0x7fffu + ((u >> 16) & 1u)) & 0xffff0000u;
    float r;
    __builtin_memcpy(&r, &u, 4);
    return r;
}

template <typename PT, typename TT>
void launch_stats(const void* pred, const void* tgt, int64_t n, double tau, int nparts, uint64_t* parts, hipStream_t s) {
    using C = typename PredOf<PT>::type;
    // the widest aligned middle: first h in [0, 64) where both operands' chunk loads are aligned (none -> all per thread)
    const uintptr_t pa = (uintptr_t)pred, ta = (uintptr_t)tgt;
    int64_t head = n;
    for (int64_t h = 0; h < 64 && h < n; ++h)
        if ((pa + h * sizeof(PT)) % vec_align<PT>() == 0 && (ta + h * sizeof(TT)) % vec_align<TT>() == 0) {
            head = h;
            break;
        }
    const int64_t nvec = (n - head) / kElems;
    C tau_c;
    if constexpr (std::is_same<PT, bf16>::value) tau_c = round_bf16(tau);
    else tau_c = (C)tau;
    hipLaunchKernelGGL((metrics_stats_kernel<PT, TT>), dim3(nparts), dim3(kThreads), 0, s, (const PT*)pred,
                       (const TT*)tgt, n, head, nvec, tau_c, parts);
}

template <typename PT>
int dispatch_target(const void* pred, const void* tgt, int tgt_dtype, int64_t n, double tau, int nparts, uint64_t* parts,
                    hipStream_t s) {
    switch (tgt_dtype) {
        case SN_F32: launch_stats<PT, float>(pred, tgt, n, tau, nparts, parts, s); break;
        case SN_F64: launch_stats<PT, double>(pred, tgt, n, tau, nparts, parts, s); break;
        case SN_BF16: launch_stats<PT, bf16>(pred, tgt, n, tau, nparts, parts, s); break;
        case SN_U8:
        case SN_OCC8: launch_stats<PT, uint8_t>(pred, tgt, n, tau, nparts, parts, s); break;
        case SN_I32: launch_stats<PT, int32_t>(pred, tgt, n, tau, nparts, parts, s); break;
        default: return dtype_error("target", tgt_dtype);
    }
    return SN_OK;
}

}  // namespace

extern "C" int sn_binary_stats(const void* pred, int pred_dtype, const void* target, int target_dtype, int64_t n,
                               double tau, double beta, void* parts_ws, uint64_t* state, uint64_t* batch, float* values,
                               sn_stream_t stream) {
    if (!pred || !target || !parts_ws || !state) return sn::fail(SN_ERR_INVALID_ARG, "sn_binary_stats: null pointer");
    if (n <= 0) return sn::fail(SN_ERR_INVALID_ARG, "sn_binary_stats: n must be positive");
    if (n > kMaxN) return sn::fail(SN_ERR_UNSUPPORTED, "sn_binary_stats: n <= 2^40");
    if (!(tau > 0.0 && tau < 1.0)) return sn::fail(SN_ERR_INVALID_ARG, "sn_binary_stats: tau must lie in (0, 1)");
    if (!(beta > 0.0 && beta < 1e150)) return sn::fail(SN_ERR_INVALID_ARG, "sn_binary_stats: beta must be positive");
    if (pred_dtype != SN_F32 && pred_dtype != SN_BF16 && pred_dtype != SN_F64) return dtype_error("pred", pred_dtype);
    if (target_dtype != SN_F32 && target_dtype != SN_F64 && target_dtype != SN_BF16 && target_dtype != SN_U8 &&
        target_dtype != SN_OCC8 && target_dtype != SN_I32)
        return dtype_error("target", target_dtype);
    const size_t psz = pred_dtype == SN_F64 ? 8 : (pred_dtype == SN_F32 ? 4 : 2);
    const size_t tsz = (target_dtype == SN_F64) ? 8 : (target_dtype == SN_U8 || target_dtype == SN_OCC8) ? 1
                       : (target_dtype == SN_BF16) ? 2 : 4;
    if ((uintptr_t)pred % psz || (uintptr_t)target % tsz)
        return sn::fail(SN_ERR_INVALID_ARG, "sn_binary_stats: pred / target must be aligned to their element size");
    if ((uintptr_t)parts_ws % 8 || (uintptr_t)state % 8 || (uintptr_t)batch % 8 || (uintptr_t)values % 4)
        return sn::fail(SN_ERR_INVALID_ARG, "sn_binary_stats: parts_ws / state / batch must be 8-byte, values 4-byte aligned");
    hipStream_t s = sn::as_stream(stream);
    // two chunks per lane per workgroup at least, SN_METRIC_MAX_PARTS workgroups at most
    const int64_t want = (n + 2 * kChunk - 1) / (2 * kChunk);
    const int nparts = (int)(want < SN_METRIC_MAX_PARTS ? want : SN_METRIC_MAX_PARTS);
    uint64_t* parts = static_cast<uint64_t*>(parts_ws);
    int rc = SN_OK;
    switch (pred_dtype) {
        case SN_F32: rc = dispatch_target<float>(pred, target, target_dtype, n, tau, nparts, parts, s); break;
        case SN_BF16: rc = dispatch_target<bf16>(pred, target, target_dtype, n, tau, nparts, parts, s); break;
        default: rc = dispatch_target<double>(pred, target, target_dtype, n, tau, nparts, parts, s); break;
    }
    if (rc) return rc;
    if (int e = sn::check_launch("sn_binary_stats(stats)")) return e;
    hipLaunchKernelGGL(metrics_combine_kernel, dim3(1), dim3(kCombineThreads), 0, s, parts, nparts, n, beta, state, batch,
                       values);
    return sn::check_launch("sn_binary_stats(combine)");
}


// ---------------------------------------------------------------------------------------------------------------------
// K6 curve -- the same counting at T thresholds in ONE pass (sn_binary_curve).  Every prediction is binned by the number
// of (rounded) thresholds it clears, split by target class; the confusion counts at threshold k are suffix sums of that
// histogram, formed on the host.  The two end bins -- below the first threshold (relu zeros: most of a real batch) and
// at or above the last (a saturated tanh) -- are counted in registers, a wave at a time (lane masks and population
// counts); only what lies between goes through a branch-free binary search over an LDS table and an LDS integer add into
// the wave's own copy of the histogram, so the cell that holds most of a real batch is never an LDS address.
// Per-workgroup partial histograms leave as u32 with plain stores; a second launch sums them and adds into the caller's
// u64 state.  A workgroup never straddles two segments.
//
// Bound: HBM by bytes (the same bytes as sn_binary_stats, read once); measured, the search's vector instructions and
// LDS round trips keep the pass at 0.38 of the copy rate at T = 20.
namespace {

constexpr int kCurveBins = 256;                 // LDS bins per class: T + 1 <= 256
constexpr int kCurveRows = 64, kCurveCells = 4;   // combine: 4 cells x 64 rows of partial records per workgroup
constexpr int kMaxSegments = 1 << 20;
static_assert(SN_CURVE_MAX_THRESHOLDS < kCurveBins && kThreads == kCurveBins, "one table slot per thread");

template <typename C>
struct CurveThresholds {
    C v[SN_CURVE_MAX_THRESHOLDS];
};

struct CurveRegs {
    uint32_t lo_all, lo_pos, hi_all, hi_pos, bad_pred, bad_tgt;
};

// N elements of one lane.  The end bins and the bad values are counted across the wave (a comparison leaves its lane mask
// in scalar registers; the population counts run on the scalar unit): every counter holds the WAVE's total in each lane
// that is still active, and lane 0 -- which holds the lowest index of its wave and so leaves every loop last -- reports
// it.  thr[0 .. 2^STEPS) is the table padded with +Inf; hist is this wave's [2][kCurveBins] copy.  STEPS = 0 (T = 1):
// the two end bins are all there is.
template <int N, int STEPS, typename PT, typename TT>
__device__ __forceinline__ void bin_elems(const PT* pv, const TT* tv, typename PredOf<PT>::type t_first,
                                          typename PredOf<PT>::type t_last, const typename PredOf<PT>::type* thr,
                                          uint32_t* hist, CurveRegs& c) {
    using C = typename PredOf<PT>::type;
    C p[N];
    bool tt[N], mid[N], any = false;
#pragma unroll
    for (int j = 0; j < N; ++j) {
        p[j] = (C)pv[j];
        bool bt;
        classify_target(tv[j], tt[j], bt);
        const bool lo = !(p[j] >= t_first), hi = p[j] >= t_last;   // NaN clears no threshold: bin 0
        const unsigned long long m_tt = __ballot(tt[j]), m_lo = __ballot(lo), m_hi = __ballot(hi);
        c.lo_all += __popcll(m_lo);
        c.lo_pos += __popcll(m_lo & m_tt);
        c.hi_all += __popcll(m_hi);
        c.hi_pos += __popcll(m_hi & m_tt);
        c.bad_pred += __popcll(__ballot((p[j] < (C)0) || (p[j] > (C)1)));
        c.bad_tgt += __popcll(__ballot(bt));
        mid[j] = !lo && !hi;
        any |= mid[j];
    }
    if constexpr (STEPS > 0) {
        if (!__any(any)) return;
        // bin = number of thresholds <= p; every lane searches (indices stay below 2^STEPS <= kCurveBins), mid lanes add
        int b[N];
#pragma unroll
        for (int j = 0; j < N; ++j) b[j] = 0;
#pragma unroll
        for (int s = STEPS - 1; s >= 0; --s)
#pragma unroll
            for (int j = 0; j < N; ++j) b[j] += thr[b[j] + (1 << s) - 1] <= p[j] ? (1 << s) : 0;
#pragma unroll
        for (int j = 0; j < N; ++j)
            if (mid[j]) atomicAdd(&hist[(int)tt[j] * kCurveBins + b[j]], 1u);
    }
}

// Partial record of workgroup w = (segment, part): parts[w * L + {cls * (T + 1) + bin | 2 * (T + 1) + {0: bad_pred,
// 1: bad_tgt}}], L = 2 * (T + 1) + 2, u32 (a workgroup counts fewer than 2^32 elements).  The split of a segment into
// head / aligned middle / tail is sn_binary_stats' own, taken per segment on the device (a segment of odd length
// starts wherever it starts).
template <int STEPS, typename PT, typename TT>
__global__ __launch_bounds__(kThreads) void curve_hist_kernel(const PT* __restrict__ pred, const TT* __restrict__ tgt,
                                                              int64_t n, int pps, int T,
                                                              CurveThresholds<typename PredOf<PT>::type> th,
                                                              uint32_t* __restrict__ parts) {
    using C = typename PredOf<PT>::type;
    __shared__ uint32_t hist[kThreads / 64][2][kCurveBins];
    __shared__ C thr[kCurveBins];
    __shared__ uint32_t wsum[kThreads / 64][6];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int seg = blockIdx.x / pps, part = blockIdx.x - seg * pps;
    for (int i = tid; i < (kThreads / 64) * 2 * kCurveBins; i += kThreads) (&hist[0][0][0])[i] = 0u;
    thr[tid] = tid < T ? th.v[tid] : (C)__builtin_inf();
    __syncthreads();
    const C t_first = thr[0], t_last = thr[T - 1];

    pred += (int64_t)seg * n;
    tgt += (int64_t)seg * n;
    const uintptr_t pa = (uintptr_t)pred, ta = (uintptr_t)tgt;
    int64_t head = n;
    for (int64_t h = 0; h < 64 && h < n; ++h)
        if ((pa + h * sizeof(PT)) % vec_align<PT>() == 0 && (ta + h * sizeof(TT)) % vec_align<TT>() == 0) {
            head = h;
            break;
        }
    const int64_t nvec = (n - head) / kElems;

    CurveRegs c{0, 0, 0, 0, 0, 0};
    uint32_t* hw = &hist[wave][0][0];
    const int64_t gtid = (int64_t)part * kThreads + tid, gstride = (int64_t)pps * kThreads;
    const PT* p = pred + head;
    const TT* t = tgt + head;
    // two chunks in flight per lane, then one, while the WHOLE wave has them (the wave's last lane decides, so that lane 0
    // takes part in every step its wave takes); what is left is one ragged step of the wave's leading lanes
    const int64_t wlast = (int64_t)part * kThreads + __builtin_amdgcn_readfirstlane(wave) * 64 + 63;
    int64_t v = gtid, vl = wlast;
    for (; vl + gstride < nvec; v += 2 * gstride, vl += 2 * gstride) {
        const Chunk<PT> pa2 = load_chunk(p + v * kElems), pb = load_chunk(p + (v + gstride) * kElems);
        const Chunk<TT> ta2 = load_chunk(t + v * kElems), tb = load_chunk(t + (v + gstride) * kElems);
        bin_elems<kElems, STEPS, PT, TT>(pa2.v, ta2.v, t_first, t_last, thr, hw, c);
        bin_elems<kElems, STEPS, PT, TT>(pb.v, tb.v, t_first, t_last, thr, hw, c);
    }
    if (vl < nvec) {
        const Chunk<PT> pa2 = load_chunk(p + v * kElems);
        const Chunk<TT> ta2 = load_chunk(t + v * kElems);
        bin_elems<kElems, STEPS, PT, TT>(pa2.v, ta2.v, t_first, t_last, thr, hw, c);
        v += gstride;
    }
    if (v < nvec) {
        const Chunk<PT> pa2 = load_chunk(p + v * kElems);
        const Chunk<TT> ta2 = load_chunk(t + v * kElems);
        bin_elems<kElems, STEPS, PT, TT>(pa2.v, ta2.v, t_first, t_last, thr, hw, c);
    }
    for (int64_t i = gtid; i < head; i += gstride)
        bin_elems<1, STEPS, PT, TT>(pred + i, tgt + i, t_first, t_last, thr, hw, c);
    for (int64_t i = head + nvec * kElems + gtid; i < n; i += gstride)
        bin_elems<1, STEPS, PT, TT>(pred + i, tgt + i, t_first, t_last, thr, hw, c);

    const uint32_t w[6] = {c.lo_all, c.lo_pos, c.hi_all, c.hi_pos, c.bad_pred, c.bad_tgt};   // lane 0: the wave's totals
    if (lane == 0)
#pragma unroll
        for (int k = 0; k < 6; ++k) wsum[wave][k] = w[k];
    __syncthreads();   // the waves' LDS adds have landed too
    const int nb = T + 1, L = 2 * nb + 2;
    uint32_t* rec = parts + (size_t)blockIdx.x * L;
    for (int cell = tid; cell < L; cell += kThreads) {
        uint32_t s = 0;
        if (cell >= 2 * nb) {
            for (int q = 0; q < kThreads / 64; ++q) s += wsum[q][4 + cell - 2 * nb];
        } else {
            const int cls = cell >= nb, b = cell - cls * nb;
            if (b == 0 || b == T) {   // the register-counted end bins (T == 1: these are all there is)
                const int k = b == 0 ? 0 : 2;
                uint32_t all = 0, pos = 0;
                for (int q = 0; q < kThreads / 64; ++q) all += wsum[q][k], pos += wsum[q][k + 1];
                s = cls ? pos : all - pos;
            } else {
                for (int q = 0; q < kThreads / 64; ++q) s += hist[q][cls][b];
            }
        }
        rec[cell] = s;
    }
}

// state[seg * L + cell] += sum over the segment's parts; batch (nullable) receives the sum itself.  A workgroup takes
// kCurveCells cells of one segment: kCurveRows threads per cell, each with its loads in flight eight at a time.
__global__ __launch_bounds__(kCurveRows * kCurveCells) void curve_combine_kernel(const uint32_t* __restrict__ parts,
                                                                                int pps, int L, int blocks_per_seg,
                                                                                uint64_t* __restrict__ state,
                                                                                uint64_t* __restrict__ batch) {
    __shared__ uint64_t sh[kCurveRows][kCurveCells];
    const int tid = threadIdx.x, col = tid % kCurveCells, row = tid / kCurveCells;
    const int seg = blockIdx.x / blocks_per_seg;
    const int cell = (blockIdx.x - seg * blocks_per_seg) * kCurveCells + col;
    uint64_t s = 0;
    if (cell < L) {
        const uint32_t* src = parts + (size_t)seg * pps * L + cell;
        for (int q = row; q < pps; q += 8 * kCurveRows) {
            uint32_t v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = q + u * kCurveRows < pps ? src[(size_t)(q + u * kCurveRows) * L] : 0u;
#pragma unroll
            for (int u = 0; u < 8; ++u) s += v[u];
        }
    }
    sh[row][col] = s;
    __syncthreads();
    for (int h = kCurveRows / 2; h > 0; h >>= 1) {
        if (row < h) sh[row][col] += sh[row + h][col];
        __syncthreads();
    }
    if (row != 0 || cell >= L) return;
    const size_t at = (size_t)seg * L + cell;
    state[at] += sh[0][col];
    if (batch) batch[at] = sh[0][col];
}

// workgroups per segment: two chunks per lane at least, SN_METRIC_MAX_PARTS workgroups over all segments at most
int curve_parts_per_segment(int64_t n, int S) {
    const int64_t want = (n + 2 * kChunk - 1) / (2 * kChunk);
    const int64_t cap = SN_METRIC_MAX_PARTS / S > 0 ? SN_METRIC_MAX_PARTS / S : 1;
    return (int)(want < cap ? want : cap);
}

int curve_dtype_error(const char* what, int dt) {
    return sn::fail(dt >= SN_F32 && dt <= SN_I32 ? SN_ERR_UNSUPPORTED : SN_ERR_INVALID_ARG,
                    "sn_binary_curve: %s dtype %d not accepted (pred: SN_F32 | SN_BF16 | SN_F64; target: SN_F32 | SN_F64 | "
                    "SN_BF16 | SN_U8 | SN_OCC8 | SN_I32)", what, dt);
}

bool curve_shape_ok(int64_t n, int S, int T) {
    return n > 0 && S > 0 && S <= kMaxSegments && T >= 1 && T <= SN_CURVE_MAX_THRESHOLDS && n <= kMaxN / S;
}

template <typename PT, typename TT>
void launch_curve(const void* pred, const void* tgt, int64_t n, int S, const double* thr_host, int T, int pps,
                  uint32_t* parts, hipStream_t s) {
    using C = typename PredOf<PT>::type;
    CurveThresholds<C> th;
    for (int k = 0; k < SN_CURVE_MAX_THRESHOLDS; ++k) {
        const double tau = k < T ? thr_host[k] : 2.0;
        if constexpr (std::is_same<PT, bf16>::value) th.v[k] = round_bf16(tau);
        else th.v[k] = (C)tau;
    }
    // steps of the search over a table of 2^steps > T slots: none at T = 1, 5 up to T = 31, 8 up to the cap
    const dim3 grid((unsigned)(S * pps)), block(kThreads);
    if (T == 1)
        hipLaunchKernelGGL((curve_hist_kernel<0, PT, TT>), grid, block, 0, s, (const PT*)pred, (const TT*)tgt, n, pps, T, th,
                           parts);
    else if (T < 32)
        hipLaunchKernelGGL((curve_hist_kernel<5, PT, TT>), grid, block, 0, s, (const PT*)pred, (const TT*)tgt, n, pps, T, th,
                           parts);
    else
        hipLaunchKernelGGL((curve_hist_kernel<8, PT, TT>), grid, block, 0, s, (const PT*)pred, (const TT*)tgt, n, pps, T, th,
                           parts);
}

template <typename PT>
int dispatch_curve_target(const void* pred, const void* tgt, int tgt_dtype, int64_t n, int S, const double* thr_host,
                          int T, int pps, uint32_t* parts, hipStream_t s) {
    switch (tgt_dtype) {
        case SN_F32: launch_curve<PT, float>(pred, tgt, n, S, thr_host, T, pps, parts, s); break;
        case SN_F64: launch_curve<PT, double>(pred, tgt, n, S, thr_host, T, pps, parts, s); break;
        case SN_BF16: launch_curve<PT, bf16>(pred, tgt, n, S, thr_host, T, pps, parts, s); break;
        case SN_U8:
        case SN_OCC8: launch_curve<PT, uint8_t>(pred, tgt, n, S, thr_host, T, pps, parts, s); break;
        default: launch_curve<PT, int32_t>(pred, tgt, n, S, thr_host, T, pps, parts, s); break;
    }
    return SN_OK;
}

}  // namespace

extern "C" size_t sn_binary_curve_ws_bytes(int64_t n, int S, int T) {
    if (!curve_shape_ok(n, S, T)) return 0;
    return (size_t)S * curve_parts_per_segment(n, S) * (2 * (T + 1) + 2) * sizeof(uint32_t);
}

extern "C" int sn_binary_curve(const void* pred, int pred_dtype, const void* target, int target_dtype, int64_t n, int S,
                               const double* thresholds_host, int T, void* parts_ws, size_t ws_bytes, uint64_t* state,
                               uint64_t* batch, sn_stream_t stream) {
    if (!pred || !target || !thresholds_host || !parts_ws || !state)
        return sn::fail(SN_ERR_INVALID_ARG, "sn_binary_curve: null pointer");
    if (n <= 0) return sn::fail(SN_ERR_INVALID_ARG, "sn_binary_curve: n must be positive");
    if (S <= 0) return sn::fail(SN_ERR_INVALID_ARG, "sn_binary_curve: S must be positive");
    if (T < 1 || T > SN_CURVE_MAX_THRESHOLDS)
        return sn::fail(SN_ERR_INVALID_ARG, "sn_binary_curve: T must lie in [1, %d] (got %d)", SN_CURVE_MAX_THRESHOLDS, T);
    if (!curve_shape_ok(n, S, T)) return sn::fail(SN_ERR_UNSUPPORTED, "sn_binary_curve: S <= 2^20 and S * n <= 2^40");
    for (int k = 0; k < T; ++k) {
        if (!(thresholds_host[k] > 0.0 && thresholds_host[k] < 1.0))
            return sn::fail(SN_ERR_INVALID_ARG, "sn_binary_curve: thresholds must lie in (0, 1) (entry %d)", k);
        if (k > 0 && !(thresholds_host[k] > thresholds_host[k - 1]))
            return sn::fail(SN_ERR_INVALID_ARG, "sn_binary_curve: thresholds must be strictly increasing (entry %d)", k);
    }
    if (pred_dtype != SN_F32 && pred_dtype != SN_BF16 && pred_dtype != SN_F64) return curve_dtype_error("pred", pred_dtype);
    if (target_dtype != SN_F32 && target_dtype != SN_F64 && target_dtype != SN_BF16 && target_dtype != SN_U8 &&
        target_dtype != SN_OCC8 && target_dtype != SN_I32)
        return curve_dtype_error("target", target_dtype);
    const size_t psz = pred_dtype == SN_F64 ? 8 : (pred_dtype == SN_F32 ? 4 : 2);
    const size_t tsz = (target_dtype == SN_F64) ? 8 : (target_dtype == SN_U8 || target_dtype == SN_OCC8) ? 1
                       : (target_dtype == SN_BF16) ? 2 : 4;
    if ((uintptr_t)pred % psz || (uintptr_t)target % tsz)
        return sn::fail(SN_ERR_INVALID_ARG, "sn_binary_curve: pred / target must be aligned to their element size");
    if ((uintptr_t)parts_ws % 8 || (uintptr_t)state % 8 || (uintptr_t)batch % 8)
        return sn::fail(SN_ERR_INVALID_ARG, "sn_binary_curve: parts_ws / state / batch must be 8-byte aligned");
    const size_t need = sn_binary_curve_ws_bytes(n, S, T);
    if (ws_bytes < need)
        return sn::fail(SN_ERR_INVALID_ARG, "sn_binary_curve: parts_ws holds %zu bytes, %zu needed "
                        "(sn_binary_curve_ws_bytes)", ws_bytes, need);
    hipStream_t s = sn::as_stream(stream);
    const int pps = curve_parts_per_segment(n, S);
    uint32_t* parts = static_cast<uint32_t*>(parts_ws);
    switch (pred_dtype) {
        case SN_F32: dispatch_curve_target<float>(pred, target, target_dtype, n, S, thresholds_host, T, pps, parts, s); break;
        case SN_BF16: dispatch_curve_target<bf16>(pred, target, target_dtype, n, S, thresholds_host, T, pps, parts, s); break;
        default: dispatch_curve_target<double>(pred, target, target_dtype, n, S, thresholds_host, T, pps, parts, s); break;
    }
    if (int e = sn::check_launch("sn_binary_curve(histogram)")) return e;
    const int L = 2 * (T + 1) + 2, blocks_per_seg = (L + kCurveCells - 1) / kCurveCells;
    hipLaunchKernelGGL(curve_combine_kernel, dim3((unsigned)(S * blocks_per_seg)), dim3(kCurveRows * kCurveCells), 0, s,
                       parts, pps, L, blocks_per_seg, state, batch);
    return sn::check_launch("sn_binary_curve(combine)");
}
