// Rows packed by `offsets` (tile b owns rows offsets[b] .. offsets[b + 1]): which tile a row belongs to, which rows belong
// to any, and the walk over the tiles that own rows of a workgroup's chunk.  Shared by thin.hip (K17), voxel_classes.hip
// (K18), knn.hip (K21), shape.hip (K22), render.hip (K23) and voxel_pool.hip (K24): one rule, one text.  Device text only,
// no kernels.  (ingest.hip's count_bad and kitti.hip's forward scan over offsets are other rules and keep their own text.)
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace sn {

// the bit patterns the kernels store for "no value"
__device__ __forceinline__ double pos_inf() { return __longlong_as_double(0x7ff0000000000000ll); }
__device__ __forceinline__ double quiet_nan() { return __longlong_as_double(0x7ff8000000000000ll); }

// rows that tiles own: offsets[B] clamped into 0 .. total
__device__ __forceinline__ int live_rows(const int64_t* __restrict__ offsets, int B, int total) {
    const int64_t m = offsets[B];
    return m <= 0 ? 0 : (m < total ? (int)m : total);
}

// the tile of packed row i: the last b in 0 .. B-1 with offsets[b] <= i (empty tiles are skipped by construction)
__device__ __forceinline__ int tile_of_row(const int64_t* __restrict__ offsets, int B, int64_t i) {
    int lo = 0, hi = B - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (offsets[mid] <= i) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// first tile whose rows can reach row `base`: the largest b with offsets[b] <= base (0 if there is none)
__device__ __forceinline__ int tile_of(const int64_t* __restrict__ offsets, int B, int64_t base) {
    int lo = 0, hi = B;   // first b in [0, B) with offsets[b] > base
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (offsets[mid] > base) hi = mid; else lo = mid + 1;
    }
    return lo > 0 ? lo - 1 : 0;
}

// f(b, lo, hi, from, to) for every tile b that owns rows of the chunk [base, min(base + chunk, total)), in order: lo, hi
// are the tile's own offsets, from .. to its rows inside the chunk, never none.  An empty tile and one that ends before
// the chunk are skipped; the first tile that starts at or behind the chunk's end ends the walk.  The trips are a function
// of (offsets, base) alone: every lane of a workgroup takes the same ones, so f may hold barriers.
// A callback, not an iterator struct whose next() a `for` calls: with next() the skipping loop nests inside the caller's,
// its loads of offsets leave the scalar unit and every walking kernel takes 4 to 14 more VGPRs.
template <typename F>
__device__ __forceinline__ void for_tiles(const int64_t* __restrict__ offsets, int B, int64_t base, int chunk, int64_t total,
                                          F&& f) {
    const int64_t end = base + chunk < total ? base + chunk : total;
    for (int b = tile_of(offsets, B, base); b < B; ++b) {
        const int64_t lo = offsets[b], hi = offsets[b + 1];
        if (lo >= end) break;
        const int64_t from = lo > base ? lo : base, to = hi < end ? hi : end;
        if (from >= to) continue;   // an empty tile, or one that ends before the chunk
        f(b, lo, hi, from, to);
    }
}

}  // namespace sn
