// K20 -- weighted pinball (quantile) loss of the quantile ensemble: one streaming pass over (pred [B,Q,n_per], gt [B,n_per])
// gives the weighted pinball sum of every quantile and the count of every weight bin; a one-workgroup kernel turns them into
// the loss, each quantile's share and the per-bin coefficients of the gradient; a second streaming pass writes dL/dpred.
//
// Reference (what is restated, not how): core/criterions/quant_loss.py:74-102 over w_mse.py:114-145, per sample -- the
// reference's own broadcast pairs every ground truth with every sample's prediction and is its intent only at B = 1.
//
// Bound: HBM.  Algorithmic bytes per voxel: forward Q sizeof(pred) + sizeof(gt); backward the same + Q sizeof(pred) written.
// A thread reads gt once per voxel and walks the Q channels at stride n_per.  All accumulation is fp64 in a fixed order
// (per-thread strided, wave shuffle tree, waves in order, parts in order, samples in order): the loss is bit-reproducible.
#include "common.h"
#include "loss_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxQ = SN_QUANTILE_MAX_Q;

struct QArgs {
    float q[kMaxQ];     // q_i
    float qm1[kMaxQ];   // q_i - 1, formed in float32 as the reference forms it (quant_loss.py:86 on a float32 tensor)
};

// d and rho are evaluated in the promoted type of pred and gt (a byte gt promotes to pred's type)
template <typename PT, typename GT>
struct Promoted {
    using type = typename std::conditional<std::is_same<PT, double>::value || std::is_same<GT, double>::value, double,
                                           float>::type;
};

template <typename CT>
__device__ __forceinline__ CT pinball(CT q, CT qm1, CT d) {
    const CT a = q * d, b = qm1 * d;
    return (a > b || b != b) ? a : b;   // torch.max: a NaN operand gives NaN (a and b are NaN together here)
}

// ---------------------------------------------------------------- pass 1: partial sums
// grid = (parts, B); block `part` owns voxels [part*span, (part+1)*span) of sample b (span a multiple of 4).
// parts_ws [(b*parts + part)][Q + H] = { sum_v w(gt) rho_i : i < Q } { count of bin k : k < H }
// kBinary (gt is SN_OCC8, values in {0,1}): two classes, weights and counts in registers.  Otherwise the per-thread per-bin
// counts live in LDS ([bin][thread], conflict free) and the weight of a voxel is one LDS read.
template <typename PT, typename GT, bool kBinary, int Q>
__global__ __launch_bounds__(kThreads) void quantile_stats_kernel(const PT* __restrict__ pred, const GT* __restrict__ gt,
                                                                  long n_per, long span, QArgs qa,
                                                                  const float* __restrict__ ranges,
                                                                  const float* __restrict__ bin_w, int H,
                                                                  double* __restrict__ parts) {
    using CT = typename Promoted<PT, GT>::type;
    __shared__ double red[kThreads / 64][kMaxQ + kMaxBins];
    __shared__ int cnt_l[kBinary ? 1 : kMaxBins * kThreads];
    __shared__ double w_l[kMaxBins];
    __shared__ int lut[256];
    const int part = blockIdx.x, b = blockIdx.y, nparts = gridDim.x, tid = threadIdx.x;
    const long lo = (long)part * span, hi = (lo + span < n_per) ? lo + span : n_per;
    const PT* p = pred + (size_t)b * Q * n_per;
    const GT* t = gt + (size_t)b * n_per;
    BinOf<GT> bin;
    bin.init(ranges, H);
    const int lane = tid & 63, wave = tid >> 6;
    const int nstat = Q + H;
    const bool vec = (n_per % 4 == 0);  // every channel base is then 4-element aligned (host checks the pointers)
    double acc[Q];
#pragma unroll
    for (int i = 0; i < Q; ++i) acc[i] = 0.0;

    if constexpr (kBinary) {
        const int b0 = bin((GT)0), b1 = bin((GT)1);
        const double w0 = (double)bin_w[b0], w1 = (double)bin_w[b1];
        int n_all = 0, n1 = 0;
        if (vec) {
            for (long v = lo + 4 * (long)tid; v + 3 < hi; v += 4 * kThreads) {
                const Vec4<GT> tv = load4(t + v);
                Vec4<PT> pv[Q];
#pragma unroll
                for (int i = 0; i < Q; ++i) pv[i] = load4(p + (size_t)i * n_per + v);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const bool one = tv.v[j] != 0;
                    const CT tc = one ? (CT)1 : (CT)0;
                    const double w = one ? w1 : w0;
                    n_all += 1;
                    n1 += one ? 1 : 0;
#pragma unroll
                    for (int i = 0; i < Q; ++i)
                        acc[i] += w * (double)pinball<CT>((CT)qa.q[i], (CT)qa.qm1[i], tc - (CT)pv[i].v[j]);
                }
            }
        } else {
            for (long v = lo + tid; v < hi; v += kThreads) {
                const bool one = t[v] != 0;
                const CT tc = one ? (CT)1 : (CT)0;
                const double w = one ? w1 : w0;
                n_all += 1;
                n1 += one ? 1 : 0;
#pragma unroll
                for (int i = 0; i < Q; ++i)
                    acc[i] += w * (double)pinball<CT>((CT)qa.q[i], (CT)qa.qm1[i], tc - (CT)p[(size_t)i * n_per + v]);
            }
        }
        const double c1 = wave_sum((double)n1), c0 = wave_sum((double)(n_all - n1));
        if (lane == 0) {
            for (int k = 0; k < H; ++k) red[wave][Q + k] = 0.0;
            red[wave][Q + b0] += c0;
            red[wave][Q + b1] += c1;
        }
    } else {
        if constexpr (sizeof(GT) == 1) lut[tid] = bin((GT)tid);
        for (int k = 0; k < H; ++k) cnt_l[k * kThreads + tid] = 0;
        if (tid < kMaxBins) w_l[tid] = tid < H ? (double)bin_w[tid] : 0.0;
        __syncthreads();
        if (vec) {
            for (long v = lo + 4 * (long)tid; v + 3 < hi; v += 4 * kThreads) {
                const Vec4<GT> tv = load4(t + v);
                Vec4<PT> pv[Q];
#pragma unroll
                for (int i = 0; i < Q; ++i) pv[i] = load4(p + (size_t)i * n_per + v);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int k = bin_lookup(bin, lut, tv.v[j]);
                    const double w = w_l[k];
                    const CT tc = (CT)tv.v[j];
                    cnt_l[k * kThreads + tid] += 1;
#pragma unroll
                    for (int i = 0; i < Q; ++i)
                        acc[i] += w * (double)pinball<CT>((CT)qa.q[i], (CT)qa.qm1[i], tc - (CT)pv[i].v[j]);
                }
            }
        } else {
            for (long v = lo + tid; v < hi; v += kThreads) {
                const GT tv = t[v];
                const int k = bin_lookup(bin, lut, tv);
                const double w = w_l[k];
                const CT tc = (CT)tv;
                cnt_l[k * kThreads + tid] += 1;
#pragma unroll
                for (int i = 0; i < Q; ++i)
                    acc[i] += w * (double)pinball<CT>((CT)qa.q[i], (CT)qa.qm1[i], tc - (CT)p[(size_t)i * n_per + v]);
            }
        }
        for (int k = 0; k < H; ++k) {
            const double c = wave_sum((double)cnt_l[k * kThreads + tid]);
            if (lane == 0) red[wave][Q + k] = c;
        }
    }
#pragma unroll
    for (int i = 0; i < Q; ++i) {
        const double a = wave_sum(acc[i]);
        if (lane == 0) red[wave][i] = a;
    }
    __syncthreads();
    if (tid < nstat) {
        double s = 0;
        for (int w = 0; w < kThreads / 64; ++w) s += red[w][tid];
        parts[((size_t)b * nparts + part) * nstat + tid] = s;
    }
}

// ---------------------------------------------------------------- one workgroup: parts -> stats -> loss + coefficients
// stats [B][Q + H] = the parts of a sample summed in order; tot = the samples summed in order;
// sum_w = sum_k count_k bin_w[k];  loss[1 + i] = tot_i / sum_w;  loss[0] = (sum_i tot_i) / sum_w;  coef[k] = bin_w[k] / sum_w
__global__ __launch_bounds__(kThreads) void quantile_combine_kernel(const double* __restrict__ parts, int B, int nparts, int Q,
                                                                    int H, const float* __restrict__ bin_w,
                                                                    double* __restrict__ stats, double* __restrict__ loss,
                                                                    float* __restrict__ loss32, double* __restrict__ coef) {
    __shared__ double tot[kMaxQ + kMaxBins];
    const int nstat = Q + H;
    for (int i = threadIdx.x; i < B * nstat; i += kThreads) {
        const int b = i / nstat, j = i % nstat;
        const double* src = parts + (size_t)b * nparts * nstat + j;
        double s = 0;
        int q = 0;
        for (; q + 8 <= nparts; q += 8) {   // 8 independent loads in flight, summed in order
            double v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = src[(size_t)(q + u) * nstat];
#pragma unroll
            for (int u = 0; u < 8; ++u) s += v[u];
        }
        for (; q < nparts; ++q) s += src[(size_t)q * nstat];
        stats[i] = s;
    }
    __syncthreads();  // stats[] written by this block is visible to it after the barrier
    if ((int)threadIdx.x < nstat) {
        double s = 0;
        int b = 0;
        for (; b + 8 <= B; b += 8) {
            double v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = stats[(size_t)(b + u) * nstat + threadIdx.x];
#pragma unroll
            for (int u = 0; u < 8; ++u) s += v[u];
        }
        for (; b < B; ++b) s += stats[(size_t)b * nstat + threadIdx.x];
        tot[threadIdx.x] = s;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double sum_w = 0, num = 0;
        for (int k = 0; k < H; ++k) sum_w += tot[Q + k] * (double)bin_w[k];
        for (int i = 0; i < Q; ++i) num += tot[i];
        loss[0] = num / sum_w;
        for (int i = 0; i < Q; ++i) loss[1 + i] = tot[i] / sum_w;
        if (loss32)
            for (int i = 0; i <= Q; ++i) loss32[i] = (float)loss[i];
        for (int k = 0; k < H; ++k) coef[k] = (double)bin_w[k] / sum_w;
    }
}

// ---------------------------------------------------------------- pass 2: dL/dpred
// grad[b,i,v] = up coef[bin(gt)] g,  g = -q_i (gt > pred), 1 - q_i (gt < pred), 0.5 - q_i (gt == pred: torch.max hands half
// of the gradient to each argument at a tie); 1 - q_i is -(q_i - 1) of the float32 q_i - 1, as autograd forms it.
template <typename PT, typename GT, bool kBinary, int Q>
__global__ __launch_bounds__(kThreads) void quantile_grad_kernel(const PT* __restrict__ pred, const GT* __restrict__ gt,
                                                                 long n_per, long span, QArgs qa,
                                                                 const float* __restrict__ ranges, int H,
                                                                 const double* __restrict__ coef,
                                                                 const double* __restrict__ upstream,
                                                                 const float* __restrict__ upstream32,
                                                                 PT* __restrict__ grad) {
    using CT = typename Promoted<PT, GT>::type;
    __shared__ PT ck[kMaxBins];
    __shared__ int lut[256];
    const int part = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const long lo = (long)part * span, hi = (lo + span < n_per) ? lo + span : n_per;
    const PT* p = pred + (size_t)b * Q * n_per;
    const GT* t = gt + (size_t)b * n_per;
    PT* g = grad + (size_t)b * Q * n_per;
    BinOf<GT> bin;
    bin.init(ranges, H);
    const double up = upstream ? *upstream : (upstream32 ? (double)*upstream32 : 1.0);
    PT gpos[Q], gneg[Q], gtie[Q];   // the three values of g, in pred's dtype
#pragma unroll
    for (int i = 0; i < Q; ++i) {
        gpos[i] = (PT)(-qa.q[i]);
        gneg[i] = (PT)(-qa.qm1[i]);
        gtie[i] = (PT)0.5 * gpos[i] + (PT)0.5 * gneg[i];
    }
    PT c0 = 0, c1 = 0;
    if constexpr (kBinary) {
        c0 = (PT)(coef[bin((GT)0)] * up);
        c1 = (PT)(coef[bin((GT)1)] * up);
    } else {
        if (tid < kMaxBins) ck[tid] = tid < H ? (PT)(coef[tid] * up) : (PT)0;
        if constexpr (sizeof(GT) == 1) lut[tid] = bin((GT)tid);
        __syncthreads();
    }
    auto weight = [&](GT tv) -> PT {
        if constexpr (kBinary) return (tv != 0) ? c1 : c0;
        else return ck[bin_lookup(bin, lut, tv)];
    };
    auto target = [&](GT tv) -> CT {
        if constexpr (kBinary) return (tv != 0) ? (CT)1 : (CT)0;
        else return (CT)tv;
    };
    if (n_per % 4 == 0) {
        for (long v = lo + 4 * (long)tid; v + 3 < hi; v += 4 * kThreads) {
            const Vec4<GT> tv = load4(t + v);
            Vec4<PT> pv[Q];
#pragma unroll
            for (int i = 0; i < Q; ++i) pv[i] = load4(p + (size_t)i * n_per + v);
            PT c[4];
            CT tc[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) c[j] = weight(tv.v[j]), tc[j] = target(tv.v[j]);
#pragma unroll
            for (int i = 0; i < Q; ++i) {
                Vec4<PT> r;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const CT pc = (CT)pv[i].v[j];
                    r.v[j] = c[j] * (tc[j] > pc ? gpos[i] : (tc[j] < pc ? gneg[i] : gtie[i]));
                }
                store4(g + (size_t)i * n_per + v, r);
            }
        }
    } else {
        for (long v = lo + tid; v < hi; v += kThreads) {
            const GT tv = t[v];
            const PT c = weight(tv);
            const CT tc = target(tv);
#pragma unroll
            for (int i = 0; i < Q; ++i) {
                const CT pc = (CT)p[(size_t)i * n_per + v];
                g[(size_t)i * n_per + v] = c * (tc > pc ? gpos[i] : (tc < pc ? gneg[i] : gtie[i]));
            }
        }
    }
}

int check_common(const char* fn, const void* pred, int pred_dtype, const void* gt, int gt_dtype, int B, int Q, int64_t n_per,
                 const float* qs, const float* ranges, int H, QArgs* qa) {
    if (!pred || !gt || !qs || !ranges) return sn::fail(SN_ERR_INVALID_ARG, "%s: null pointer", fn);
    if (B <= 0 || n_per <= 0) return sn::fail(SN_ERR_INVALID_ARG, "%s: B and n_per must be positive", fn);
    if (Q < 1 || Q > kMaxQ) return sn::fail(SN_ERR_INVALID_ARG, "%s: 1 <= Q <= %d quantiles", fn, kMaxQ);
    if (H < 1 || H > kMaxBins) return sn::fail(SN_ERR_INVALID_ARG, "%s: 1 <= H <= %d bins", fn, kMaxBins);
    if (pred_dtype != SN_F32 && pred_dtype != SN_F64 && pred_dtype != SN_BF16)
        return sn::fail(SN_ERR_INVALID_ARG, "%s: pred must be SN_F32 or SN_F64", fn);
    if (gt_dtype != SN_F32 && gt_dtype != SN_F64 && gt_dtype != SN_U8 && gt_dtype != SN_OCC8)
        return sn::fail(SN_ERR_INVALID_ARG, "%s: bad gt dtype %d", fn, gt_dtype);
    if (pred_dtype == SN_BF16)
        return sn::fail(SN_ERR_UNSUPPORTED, "%s: bf16 predictions are not served (the ensemble returns float32)", fn);
    for (int i = 0; i < kMaxQ; ++i) {
        const float q = i < Q ? qs[i] : 0.5f;
        if (!(q > 0.0f && q < 1.0f)) return sn::fail(SN_ERR_UNSUPPORTED, "%s: quantile %d = %g is outside (0, 1)", fn, i, q);
        qa->q[i] = q;
        qa->qm1[i] = q - 1.0f;
    }
    if (B > 65535) return sn::fail(SN_ERR_UNSUPPORTED, "%s: B <= 65535", fn);
    const size_t ga = (gt_dtype == SN_F64 || gt_dtype == SN_F32) ? 16 : 4;
    if (n_per % 4 == 0 && (((uintptr_t)pred % 16) || ((uintptr_t)gt % ga)))
        return sn::fail(SN_ERR_INVALID_ARG, "%s: pred / gt must be 16-byte (byte gt: 4-byte) aligned", fn);
    return SN_OK;
}

// span per part: a multiple of 4 so that the vector loop of every part starts aligned
long span_of(int64_t n_per, int nparts) {
    long s = (long)((n_per + nparts - 1) / nparts);
    return (s + 3) / 4 * 4;
}

}  // namespace

#define SN_Q_TYPES(KERNEL, QN)                                                                                    \
    do {                                                                                                          \
        if (pred_dtype == SN_F32) {                                                                               \
            if (gt_dtype == SN_F32) KERNEL(float, float, false, QN);                                              \
            else if (gt_dtype == SN_F64) KERNEL(float, double, false, QN);                                        \
            else if (gt_dtype == SN_OCC8) KERNEL(float, uint8_t, true, QN);                                       \
            else KERNEL(float, uint8_t, false, QN);                                                               \
        } else {                                                                                                  \
            if (gt_dtype == SN_F32) KERNEL(double, float, false, QN);                                             \
            else if (gt_dtype == SN_F64) KERNEL(double, double, false, QN);                                       \
            else if (gt_dtype == SN_OCC8) KERNEL(double, uint8_t, true, QN);                                      \
            else KERNEL(double, uint8_t, false, QN);                                                              \
        }                                                                                                         \
    } while (0)

#define SN_Q_DISPATCH(KERNEL)                                                                                     \
    switch (Q) {                                                                                                  \
        case 1: SN_Q_TYPES(KERNEL, 1); break;                                                                     \
        case 2: SN_Q_TYPES(KERNEL, 2); break;                                                                     \
        case 3: SN_Q_TYPES(KERNEL, 3); break;                                                                     \
        case 4: SN_Q_TYPES(KERNEL, 4); break;                                                                     \
        case 5: SN_Q_TYPES(KERNEL, 5); break;                                                                     \
        case 6: SN_Q_TYPES(KERNEL, 6); break;                                                                     \
        case 7: SN_Q_TYPES(KERNEL, 7); break;                                                                     \
        default: SN_Q_TYPES(KERNEL, 8); break;                                                                    \
    }

extern "C" int sn_quantile_forward(const void* pred, int pred_dtype, const void* gt, int gt_dtype, int B, int Q,
                                   int64_t n_per, const float* qs, const float* ranges, const float* bin_w, int H,
                                   double* parts_ws, double* stats, double* loss, float* loss_f32, double* coef,
                                   sn_stream_t stream) {
    if (!bin_w || !parts_ws || !stats || !loss || !coef)
        return sn::fail(SN_ERR_INVALID_ARG, "sn_quantile_forward: null pointer");
    QArgs qa;
    if (int rc = check_common("sn_quantile_forward", pred, pred_dtype, gt, gt_dtype, B, Q, n_per, qs, ranges, H, &qa))
        return rc;
    hipStream_t s = sn::as_stream(stream);
    const int nparts = SN_QUANTILE_PARTS(n_per);
    const long span = span_of(n_per, nparts);
#define SN_QSTATS(PT, GT, BIN, QN)                                                                                \
    hipLaunchKernelGGL((quantile_stats_kernel<PT, GT, BIN, QN>), dim3(nparts, B), dim3(kThreads), 0, s,           \
                       (const PT*)pred, (const GT*)gt, (long)n_per, span, qa, ranges, bin_w, H, parts_ws)
    SN_Q_DISPATCH(SN_QSTATS)
#undef SN_QSTATS
    if (int rc = sn::check_launch("sn_quantile_forward(stats)")) return rc;
    hipLaunchKernelGGL(quantile_combine_kernel, dim3(1), dim3(kThreads), 0, s, parts_ws, B, nparts, Q, H, bin_w, stats, loss,
                       loss_f32, coef);
    return sn::check_launch("sn_quantile_forward(combine)");
}

extern "C" int sn_quantile_backward(const void* pred, int pred_dtype, const void* gt, int gt_dtype, int B, int Q,
                                    int64_t n_per, const float* qs, const float* ranges, int H, const double* coef,
                                    const void* upstream_v, int up_dtype, void* grad_pred, sn_stream_t stream) {
    if (!coef || !grad_pred) return sn::fail(SN_ERR_INVALID_ARG, "sn_quantile_backward: null pointer");
    QArgs qa;
    if (int rc = check_common("sn_quantile_backward", pred, pred_dtype, gt, gt_dtype, B, Q, n_per, qs, ranges, H, &qa))
        return rc;
    if (upstream_v && up_dtype != SN_F64 && up_dtype != SN_F32)
        return sn::fail(SN_ERR_INVALID_ARG, "sn_quantile_backward: up_dtype %d (SN_F64 | SN_F32)", up_dtype);
    const double* upstream = (upstream_v && up_dtype == SN_F64) ? static_cast<const double*>(upstream_v) : nullptr;
    const float* upstream32 = (upstream_v && up_dtype == SN_F32) ? static_cast<const float*>(upstream_v) : nullptr;
    if (n_per % 4 == 0 && ((uintptr_t)grad_pred % 16))
        return sn::fail(SN_ERR_INVALID_ARG, "sn_quantile_backward: grad_pred must be 16-byte aligned");
    hipStream_t s = sn::as_stream(stream);
    const int nparts = SN_QUANTILE_BWD_PARTS(n_per);
    const long span = span_of(n_per, nparts);
#define SN_QGRAD(PT, GT, BIN, QN)                                                                                 \
    hipLaunchKernelGGL((quantile_grad_kernel<PT, GT, BIN, QN>), dim3(nparts, B), dim3(kThreads), 0, s,            \
                       (const PT*)pred, (const GT*)gt, (long)n_per, span, qa, ranges, H, coef, upstream, upstream32, \
                       (PT*)grad_pred)
    SN_Q_DISPATCH(SN_QGRAD)
#undef SN_QGRAD
    return sn::check_launch("sn_quantile_backward");
}
