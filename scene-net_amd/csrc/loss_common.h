// Device helpers of the criterion kernels, shared by loss.hip (K5) and quantile.hip (K20): the 4-wide loads and stores,
// the weight bin of a target (the reference's first-minimum search, or a 256-entry table for byte targets) and the wave
// sum of the fixed-order fp64 reductions: one rule, one text.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <type_traits>
#include "scenenet_hip.h"

namespace {

constexpr int kMaxBins = SN_LOSS_MAX_BINS;

template <typename T>
struct Vec4 {
    T v[4];
};

template <typename T>
__device__ __forceinline__ Vec4<T> load4(const T* p) {
    Vec4<T> r;
    if constexpr (sizeof(T) == 2) {
        const uint2 u = *reinterpret_cast<const uint2*>(p);
        __builtin_memcpy(&r, &u, 8);
    } else if constexpr (sizeof(T) == 4) {
        const uint4 u = *reinterpret_cast<const uint4*>(p);
        __builtin_memcpy(&r, &u, 16);
    } else if constexpr (sizeof(T) == 8) {
        const uint4 u0 = reinterpret_cast<const uint4*>(p)[0], u1 = reinterpret_cast<const uint4*>(p)[1];
        __builtin_memcpy(&r.v[0], &u0, 16);
        __builtin_memcpy(&r.v[2], &u1, 16);
    } else {
        const uint32_t u = *reinterpret_cast<const uint32_t*>(p);
        __builtin_memcpy(&r, &u, 4);
    }
    return r;
}

template <typename T>
__device__ __forceinline__ void store4(T* p, const Vec4<T>& r) {
    if constexpr (sizeof(T) == 2) {
        uint2 u;
        __builtin_memcpy(&u, &r, 8);
        *reinterpret_cast<uint2*>(p) = u;
    } else if constexpr (sizeof(T) == 4) {
        uint4 u;
        __builtin_memcpy(&u, &r, 16);
        *reinterpret_cast<uint4*>(p) = u;
    } else {
        uint4 u0, u1;
        __builtin_memcpy(&u0, &r.v[0], 16);
        __builtin_memcpy(&u1, &r.v[2], 16);
        reinterpret_cast<uint4*>(p)[0] = u0;
        reinterpret_cast<uint4*>(p)[1] = u1;
    }
}

// w_mse.py:122 -- argmin_k |y - ranges[k]|, first minimum; arithmetic in gt's dtype promoted with the fp32 ranges
// (f64 gt: fp64; f32 gt: fp32; byte gt, our extension: fp32).
template <typename GT>
struct BinOf {
    using C = typename std::conditional<std::is_same<GT, double>::value, double, float>::type;
    C r[kMaxBins];
    int H;
    __device__ void init(const float* ranges, int h) {
        H = h;
#pragma unroll
        for (int k = 0; k < kMaxBins; ++k) r[k] = (C)ranges[k < h ? k : h - 1];
    }
    __device__ __forceinline__ int operator()(GT y) const {
        const C yy = (C)y;
        C best = fabs(yy - r[0]);
        int idx = 0;
#pragma unroll
        for (int k = 1; k < kMaxBins; ++k) {
            const C d = fabs(yy - r[k]);
            const bool lt = (k < H) && (d < best);
            best = lt ? d : best;
            idx = lt ? k : idx;
        }
        return idx;
    }
};

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// byte targets find their bin in a 256-entry LDS table, float targets by the first-minimum search of the reference
template <typename GT>
__device__ __forceinline__ int bin_lookup(const BinOf<GT>& bin, const int* lut, GT tv) {
    if constexpr (sizeof(GT) == 1) return lut[tv];
    else return bin(tv);
}

}  // namespace
