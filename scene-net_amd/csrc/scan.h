// The wave and workgroup scan, rank and reduce primitives of the kernels that compact rows in scan order, shared by
// crops.hip (K9, K12), dbscan.hip (K10), towers.hip (K8), voxel_cloud.hip (K16) and thin.hip (K17): one rule, one text.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace sn {

// the chunk of crops.hip, voxel_cloud.hip and thin.hip: one WAVE per workgroup, 16 groups of 64 consecutive rows per lane
constexpr int kWaveLanes = 64;
constexpr int kWaveGroups = 16;
constexpr int kWaveChunk = kWaveLanes * kWaveGroups;   // rows per workgroup
// ... and the workgroup that scans their per-chunk counts
constexpr int kScanThreads = 256;
constexpr int kScanItems = 8;                          // consecutive slots per thread and step of a prefix kernel

// ---------------------------------------------------------------- one wave
// v of lane j (wave-uniform j) in the wave's scalar registers
__device__ __forceinline__ uint64_t readlane64(uint64_t v, int j) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, j);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), j);
    return ((uint64_t)hi << 32) | lo;
}

// set bits of a ballot below this lane: the lane's rank among the lanes that voted
__device__ __forceinline__ int wave_rank(unsigned long long mask) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0));
}

// op over the 64 lanes by six xor-shuffles, the result in every lane; op(mine, other) is commutative and associative
template <typename T, typename F>
__device__ __forceinline__ T wave_reduce(T v, F op) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = op(v, __shfl_xor(v, off, 64));
    return v;
}

// ---------------------------------------------------------------- one workgroup
// exclusive prefix of one tile of kThreads * kItems values held kItems per thread; returns the tile's total.
// s_wave: kThreads / 64 slots of LDS, free again on return
template <int kThreads, int kItems, typename T = int64_t>
__device__ __forceinline__ T block_exclusive(T (&v)[kItems], T* s_wave) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    T sum = 0;
#pragma unroll
    for (int q = 0; q < kItems; ++q) {
        const T t = v[q];
        v[q] = sum;
        sum += t;
    }
    T incl = sum;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const T t = __shfl_up(incl, off, 64);
        if (lane >= off) incl += t;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    T before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kThreads / 64; ++w) {
        const T t = s_wave[w];
        if (w < wave) before += t;
        total += t;
    }
    __syncthreads();   // s_wave is written again by the next tile
    const T mine = before + incl - sum;
#pragma unroll
    for (int q = 0; q < kItems; ++q) v[q] += mine;
    return total;
}

// row[0 .. n) -> its exclusive prefixes, in place, tile after tile with the running total carried; returns the total
template <int kThreads, int kItems, typename T>
__device__ __forceinline__ T scan_row(T* row, int64_t n, T* s_wave) {
    T carry = 0;
    for (int64_t t0 = 0; t0 < n; t0 += kThreads * kItems) {
        const int64_t i0 = t0 + (int64_t)threadIdx.x * kItems;
        T v[kItems];
#pragma unroll
        for (int q = 0; q < kItems; ++q) v[q] = i0 + q < n ? row[i0 + q] : 0;
        const T total = block_exclusive<kThreads, kItems>(v, s_wave);
#pragma unroll
        for (int q = 0; q < kItems; ++q)
            if (i0 + q < n) row[i0 + q] = carry + v[q];
        carry += total;
    }
    return carry;
}

// offsets[k] = the totals of the rows before k, offsets[K] = all; row k's total sits at ws[k * stride + total_at]
template <int kThreads>
__device__ __forceinline__ void totals_to_offsets(const int64_t* ws, int64_t stride, int64_t total_at, int K, int64_t* offsets,
                                                  int64_t* s_wave) {
    int64_t carry = 0;
    for (int k0 = 0; k0 < K; k0 += kThreads) {
        const int k = k0 + threadIdx.x;
        int64_t v[1] = {k < K ? ws[(int64_t)k * stride + total_at] : 0};
        const int64_t total = block_exclusive<kThreads, 1>(v, s_wave);
        if (k < K) offsets[k] = carry + v[0];
        carry += total;
    }
    if (threadIdx.x == 0) offsets[K] = carry;
}

}  // namespace sn
