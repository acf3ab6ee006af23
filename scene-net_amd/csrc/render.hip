// K23 -- point clouds to images: a z-buffer point rasteriser (sn_render_splat) and the pass that turns its keys into
// pixels (sn_render_resolve).
// replaces: nothing the reference computes.  Its visualize_ply, plot_voxelgrid(plot=True), visualize_pred_vs_gt,
//           plot_centroids and visualize_batch end in a viewer window or a matplotlib 3-D scatter on the host; here the
//           coloured rows K16, K18 and K22 leave in HBM become K images of H x W pixels without leaving the device.
//
// Definition (normative, include/scenenet_hip.h).  A row of tile b is projected by every view k with view_tile[k] == b:
//   c_r = ((A[r,0]*x + A[r,1]*y) + A[r,2]*z) + A[r,3], every fp64 operation rounded once (-ffp-contract=off), the
//   perspective quotients true divisions; the accepted row's key (depth quantum << 32 | row in tile) is reduced into the
//   s x s pixels around it by unsigned 64-bit minimum.  Nearest depth wins, the lowest row among equal quanta.
//
// Shape, splat: kRenderThreads = 256 threads per workgroup, one thread per row of the packed batch, the tiles that reach
// into the workgroup's 256 rows walked one at a time (the walk of sn::for_tiles, packed_rows.h, written out), so the test
// "is view k a view of this tile" and every camera read is uniform (scalar loads).  A row is read once and kept in registers for all its views.
//   clear     keys <- all ones, count <- 0, bad_views <- 0 (one kernel, no memset node: voxel_classes.hip, zero_kernel);
//             left out with SN_RENDER_ACCUMULATE
//   splat     per pixel of a splat of s >= 2 a relaxed agent-scope load, the 64-bit atomic min only where the load shows
//             more than the row's key (the pixel only shrinks: a stale look costs a needless atomic, never a result).  At
//             s = 1 the atomic is sent without a look: [measured, profiles/render_bench.json] the look is a scattered
//             8-byte request of its own and costs what the atomic costs -- a top view of 10^7 rows, 20 rows per pixel, took
//             twice the time with it -- while the 8-byte looks of a wider splat share 64-byte lines and spare atomics that
//             contend for them.  SN_RENDER_LOOK_ALWAYS / SN_RENDER_NO_LOOK look at every size / at none (same result; for
//             timing).  count: one 32-bit atomic add per accepted row whose centre is inside the image.  Workgroup 0
//             checks the K cameras and stores the 1s of bad_views.
// Shape, resolve: one thread per pixel of the K images; the pixel's own key and, with shading, its four neighbours'.
//
// Bound: splat reads 24 B per row once; per view and accepted row it looks at s*s pixels (8 B each) and sends at most as
// many atomics.  resolve reads 8 B (40 B with shading) and writes 4 to 16 B per pixel.
#include "common.h"
#include "packed_rows.h"

namespace {

constexpr int kRenderThreads = 256;                          // rows per workgroup of the splat kernel
constexpr int kMaxB = 1 << 16;
constexpr int64_t kMaxTotal = (int64_t)1 << 33;
constexpr unsigned long long kBackground = ~0ull;
constexpr unsigned long long kMaxQuantum = 0xffffffffull;
constexpr int64_t kMaxTileRows = 0xffffffffll;               // a tile of this many rows or more is not drawn
constexpr double kTwo32 = 4294967296.0;
constexpr double kPixelLimit = 1073741824.0;                 // |px|, |py| < 2^30

// the header's list of camera rows that show nothing (every comparison is false for a NaN)
__device__ __forceinline__ bool camera_ok(const double* __restrict__ c) {
    const double kind = c[12], near = c[13], far = c[14], s = c[15];
    if (!(kind == 0.0 || kind == 1.0)) return false;
    if (!(s >= 1.0 && s <= (double)SN_RENDER_MAX_SPLAT)) return false;
    if ((double)(int)s != s) return false;
    if (!(near < far)) return false;
    if (!(far - near < __builtin_inf())) return false;
    if (kind == 1.0 && !(near > 0.0)) return false;
    return true;
}

__global__ __launch_bounds__(256) void render_clear_kernel(unsigned long long* __restrict__ keys, uint32_t* __restrict__ count,
                                                           int64_t pixels, int32_t* __restrict__ bad_views, int K) {
    const int64_t stride = (int64_t)gridDim.x * 256, first = (int64_t)blockIdx.x * 256 + threadIdx.x;
    for (int64_t i = first; i < pixels; i += stride) {
        keys[i] = kBackground;
        if (count) count[i] = 0u;
    }
    if (first < K) bad_views[first] = 0;
}

// kLook: 0 never, 1 where the view's point size is >= 2, 2 always
template <int kLook>
__global__ __launch_bounds__(kRenderThreads) void render_splat_kernel(const double* __restrict__ pts,
                                                                      const int64_t* __restrict__ offsets, int64_t total, int B,
                                                                      const double* __restrict__ cam,
                                                                      const int32_t* __restrict__ view_tile, int K, int H, int W,
                                                                      unsigned long long* __restrict__ keys,
                                                                      uint32_t* __restrict__ count,
                                                                      int32_t* __restrict__ bad_views) {
    const int t = threadIdx.x;
    if (blockIdx.x == 0 && t < K && !camera_ok(cam + (size_t)t * 16)) bad_views[t] = 1;
    const int64_t base = (int64_t)blockIdx.x * kRenderThreads;
    const int64_t end = base + kRenderThreads < total ? base + kRenderThreads : total;
    const int64_t i = base + t;
    const size_t image = (size_t)H * (size_t)W;
    // sn::for_tiles (packed_rows.h) written out: through it the splat of the C2 batch measured 1 to 2 % slower than this
    // loop, its resolve in the same runs not
    for (int b = sn::tile_of(offsets, B, base); b < B; ++b) {
        const int64_t lo = offsets[b], hi = offsets[b + 1];
        if (lo >= end) break;
        const int64_t from = lo > base ? lo : base, to = hi < end ? hi : end;
        if (from >= to) continue;   // an empty tile, or one that ends before the workgroup's rows
        const bool refused = hi - lo >= kMaxTileRows;   // its rows' indices would reach the background key
        const bool mine = i >= from && i < to;
        double x = 0.0, y = 0.0, z = 0.0;
        if (mine && !refused) {
            const double* p = pts + i * 3;
            x = p[0];
            y = p[1];
            z = p[2];
        }
        const unsigned long long j = (unsigned long long)(i - lo);
        for (int k = 0; k < K; ++k) {
            if (view_tile[k] != b) continue;
            if (refused) {
                if (t == 0) bad_views[k] = 1;
                continue;
            }
            const double* __restrict__ c = cam + (size_t)k * 16;
            if (!camera_ok(c)) continue;
            if (!mine) continue;
            const double c0 = ((c[0] * x + c[1] * y) + c[2] * z) + c[3];
            const double c1 = ((c[4] * x + c[5] * y) + c[6] * z) + c[7];
            const double d = ((c[8] * x + c[9] * y) + c[10] * z) + c[11];
            const double near = c[13], far = c[14];
            const int s = (int)c[15];
            const bool look = kLook == 2 || (kLook == 1 && s >= 2);
            double px = c0, py = c1;
            if (c[12] == 1.0) {
                px = c0 / d;
                py = c1 / d;
            }
            if (!(near <= d && d < far && fabs(px) < kPixelLimit && fabs(py) < kPixelLimit)) continue;
            const double q = floor(((d - near) / (far - near)) * kTwo32);   // 0 .. 2^32: (d - near) <= (far - near) as rounded
            const unsigned long long dq = q >= kTwo32 ? kMaxQuantum : (unsigned long long)q;
            const unsigned long long key = (dq << 32) | j;
            const int ix = (int)floor(px), iy = (int)floor(py);   // |.| <= 2^30
            unsigned long long* plane = keys + (size_t)k * image;
            const int x0 = ix - (s - 1) / 2 > 0 ? ix - (s - 1) / 2 : 0, x1 = ix + s / 2 < W - 1 ? ix + s / 2 : W - 1;
            const int y0 = iy - (s - 1) / 2 > 0 ? iy - (s - 1) / 2 : 0, y1 = iy + s / 2 < H - 1 ? iy + s / 2 : H - 1;
            for (int Y = y0; Y <= y1; ++Y) {
                for (int X = x0; X <= x1; ++X) {
                    unsigned long long* cell = plane + (size_t)Y * (size_t)W + (size_t)X;
                    if (!look || __hip_atomic_load(cell, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > key)
                        __hip_atomic_fetch_min(cell, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
            if (count && ix >= 0 && ix < W && iy >= 0 && iy < H)
                __hip_atomic_fetch_add(count + (size_t)k * image + (size_t)iy * (size_t)W + (size_t)ix, 1u, __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// (u8) floor(c * shade + 0.5): c in 0 .. 255 and shade in (0, 1], so the sum is in 0.5 .. 255.5
__device__ __forceinline__ uint32_t shaded(uint32_t c, double shade) { return (uint32_t)floor((double)c * shade + 0.5); }

__global__ __launch_bounds__(256) void render_resolve_kernel(const unsigned long long* __restrict__ keys, int K, int H, int W,
                                                             const int64_t* __restrict__ offsets, int B,
                                                             const int32_t* __restrict__ view_tile,
                                                             const uint16_t* __restrict__ rgb16, int mode, uint32_t background,
                                                             double edl, uint32_t* __restrict__ rgba, int64_t* __restrict__ index,
                                                             uint32_t* __restrict__ depth_q) {
    const int64_t image = (int64_t)H * W;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)K * image) return;
    const int k = (int)(i / image);
    const int pix = (int)(i - (int64_t)k * image);
    const int Y = pix / W, X = pix - Y * W;
    const unsigned long long key = keys[i];
    const unsigned long long dq = key >> 32, j = key & kMaxQuantum;
    // foreground: a key some row left, of a tile the batch has, at a row the tile has
    bool fore = key != kBackground;
    int64_t row = -1;
    if (fore) {
        const int b = view_tile[k];
        fore = b >= 0 && b < B;
        if (fore) {
            const int64_t lo = offsets[b], hi = offsets[b + 1];
            fore = (int64_t)j < hi - lo;
            if (fore) row = lo + (int64_t)j;
        }
    }
    uint32_t out = background;
    if (fore) {
        uint32_t r, g, bl;
        if (mode == SN_RENDER_DEPTH) {
            r = g = bl = 255u - (uint32_t)(dq >> 24);
        } else {
            const uint16_t* c = rgb16 + row * 3;
            r = c[0] >> 8;
            g = c[1] >> 8;
            bl = c[2] >> 8;
        }
        if (edl != 0.0) {
            const unsigned long long* plane = keys + (int64_t)k * image;
            long long o = 0;
            if (Y > 0) {
                const long long dn = (long long)(plane[pix - W] >> 32);
                o += (long long)dq > dn ? (long long)dq - dn : 0;
            }
            if (Y < H - 1) {
                const long long dn = (long long)(plane[pix + W] >> 32);
                o += (long long)dq > dn ? (long long)dq - dn : 0;
            }
            if (X > 0) {
                const long long dn = (long long)(plane[pix - 1] >> 32);
                o += (long long)dq > dn ? (long long)dq - dn : 0;
            }
            if (X < W - 1) {
                const long long dn = (long long)(plane[pix + 1] >> 32);
                o += (long long)dq > dn ? (long long)dq - dn : 0;
            }
            const double shade = 1.0 / (1.0 + edl * ((double)o / kTwo32));
            r = shaded(r, shade);
            g = shaded(g, shade);
            bl = shaded(bl, shade);
        }
        out = r | (g << 8) | (bl << 16) | 0xff000000u;
    }
    rgba[i] = out;
    if (index) index[i] = row;
    if (depth_q) depth_q[i] = fore ? (uint32_t)dq : 0xffffffffu;
}

int check_images(const char* what, int K, int H, int W) {
    if (K <= 0) return sn::fail(SN_ERR_INVALID_ARG, "%s: K must be positive (got %d)", what, K);
    if (H <= 0 || W <= 0) return sn::fail(SN_ERR_INVALID_ARG, "%s: H and W must be positive (got %d, %d)", what, H, W);
    if (K > SN_RENDER_MAX_VIEWS)
        return sn::fail(SN_ERR_UNSUPPORTED, "%s: K=%d beyond SN_RENDER_MAX_VIEWS = %d", what, K, SN_RENDER_MAX_VIEWS);
    if ((int64_t)H * W >= ((int64_t)1 << 31)) return sn::fail(SN_ERR_UNSUPPORTED, "%s: H * W >= 2^31", what);
    return SN_OK;
}

}  // namespace

extern "C" int sn_render_chunk_points(void) { return kRenderThreads; }

extern "C" int sn_render_splat(const double* pts, const int64_t* offsets, int64_t total, int B, const double* cam,
                               const int32_t* view_tile, int K, int H, int W, int flags, uint64_t* keys, uint32_t* count,
                               int32_t* bad_views, sn_stream_t stream) {
    const char* what = "sn_render_splat";
    if (!pts) return sn::fail(SN_ERR_INVALID_ARG, "%s: pts is null", what);
    if (!offsets) return sn::fail(SN_ERR_INVALID_ARG, "%s: offsets is null", what);
    if (!cam) return sn::fail(SN_ERR_INVALID_ARG, "%s: cam is null", what);
    if (!view_tile) return sn::fail(SN_ERR_INVALID_ARG, "%s: view_tile is null", what);
    if (!keys) return sn::fail(SN_ERR_INVALID_ARG, "%s: keys is null", what);
    if (!bad_views) return sn::fail(SN_ERR_INVALID_ARG, "%s: bad_views is null", what);
    if (total <= 0) return sn::fail(SN_ERR_INVALID_ARG, "%s: total must be positive (got %lld)", what, (long long)total);
    if (B <= 0) return sn::fail(SN_ERR_INVALID_ARG, "%s: B must be positive (got %d)", what, B);
    if (flags & ~(SN_RENDER_ACCUMULATE | SN_RENDER_NO_LOOK | SN_RENDER_LOOK_ALWAYS))
        return sn::fail(SN_ERR_INVALID_ARG, "%s: unknown flags %d", what, flags);
    if ((flags & SN_RENDER_NO_LOOK) && (flags & SN_RENDER_LOOK_ALWAYS))
        return sn::fail(SN_ERR_INVALID_ARG, "%s: flags ask for SN_RENDER_NO_LOOK and SN_RENDER_LOOK_ALWAYS at once", what);
    const int rc = check_images(what, K, H, W);
    if (rc != SN_OK) return rc;
    if (total > kMaxTotal || B > kMaxB)
        return sn::fail(SN_ERR_UNSUPPORTED, "%s: total=%lld, B=%d beyond what is served (total <= 2^33, B <= %d)", what,
                        (long long)total, B, kMaxB);
    if ((uintptr_t)pts % 8 || (uintptr_t)offsets % 8 || (uintptr_t)cam % 8 || (uintptr_t)keys % 8 || (uintptr_t)view_tile % 4 ||
        (uintptr_t)count % 4 || (uintptr_t)bad_views % 4)
        return sn::fail(SN_ERR_INVALID_ARG, "%s: pts / offsets / cam / keys must be 8-byte, view_tile / count / bad_views 4-byte aligned",
                        what);
    hipStream_t s = sn::as_stream(stream);
    unsigned long long* k64 = reinterpret_cast<unsigned long long*>(keys);
    const int64_t pixels = (int64_t)K * H * W;
    if (!(flags & SN_RENDER_ACCUMULATE)) {
        const int64_t want = (pixels + 256 * 4 - 1) / (256 * 4);
        hipLaunchKernelGGL(render_clear_kernel, dim3((unsigned)(want < 8192 ? want : 8192)), dim3(256), 0, s, k64, count, pixels,
                           bad_views, K);
    }
    const dim3 blocks((unsigned)((total + kRenderThreads - 1) / kRenderThreads)), threads(kRenderThreads);
    if (flags & SN_RENDER_NO_LOOK)
        hipLaunchKernelGGL(render_splat_kernel<0>, blocks, threads, 0, s, pts, offsets, total, B, cam, view_tile, K, H, W, k64,
                           count, bad_views);
    else if (flags & SN_RENDER_LOOK_ALWAYS)
        hipLaunchKernelGGL(render_splat_kernel<2>, blocks, threads, 0, s, pts, offsets, total, B, cam, view_tile, K, H, W, k64,
                           count, bad_views);
    else
        hipLaunchKernelGGL(render_splat_kernel<1>, blocks, threads, 0, s, pts, offsets, total, B, cam, view_tile, K, H, W, k64,
                           count, bad_views);
    return sn::check_launch(what);
}

extern "C" int sn_render_resolve(const uint64_t* keys, int K, int H, int W, const int64_t* offsets, int B,
                                 const int32_t* view_tile, const uint16_t* rgb16, int mode, uint32_t background, double edl,
                                 uint8_t* rgba, int64_t* index, uint32_t* depth_q, sn_stream_t stream) {
    const char* what = "sn_render_resolve";
    if (!keys) return sn::fail(SN_ERR_INVALID_ARG, "%s: keys is null", what);
    if (!offsets) return sn::fail(SN_ERR_INVALID_ARG, "%s: offsets is null", what);
    if (!view_tile) return sn::fail(SN_ERR_INVALID_ARG, "%s: view_tile is null", what);
    if (!rgba) return sn::fail(SN_ERR_INVALID_ARG, "%s: rgba is null", what);
    if (B <= 0) return sn::fail(SN_ERR_INVALID_ARG, "%s: B must be positive (got %d)", what, B);
    if (mode != SN_RENDER_RGB16 && mode != SN_RENDER_DEPTH) return sn::fail(SN_ERR_INVALID_ARG, "%s: unknown mode %d", what, mode);
    if (mode == SN_RENDER_RGB16 && !rgb16) return sn::fail(SN_ERR_INVALID_ARG, "%s: rgb16 is null in SN_RENDER_RGB16 mode", what);
    if (!(edl >= 0.0) || !(edl < __builtin_inf()))
        return sn::fail(SN_ERR_INVALID_ARG, "%s: edl must be finite and >= 0 (got %g)", what, edl);
    const int rc = check_images(what, K, H, W);
    if (rc != SN_OK) return rc;
    if (B > kMaxB) return sn::fail(SN_ERR_UNSUPPORTED, "%s: B=%d beyond what is served (B <= %d)", what, B, kMaxB);
    if ((uintptr_t)keys % 8 || (uintptr_t)offsets % 8 || (uintptr_t)index % 8 || (uintptr_t)view_tile % 4 || (uintptr_t)depth_q % 4 ||
        (uintptr_t)rgba % 4 || (uintptr_t)rgb16 % 2)
        return sn::fail(SN_ERR_INVALID_ARG,
                        "%s: keys / offsets / index must be 8-byte, view_tile / depth_q / rgba 4-byte, rgb16 2-byte aligned", what);
    hipStream_t s = sn::as_stream(stream);
    const int64_t pixels = (int64_t)K * H * W;
    hipLaunchKernelGGL(render_resolve_kernel, dim3((unsigned)((pixels + 255) / 256)), dim3(256), 0, s,
                       reinterpret_cast<const unsigned long long*>(keys), K, H, W, offsets, B, view_tile, rgb16, mode, background,
                       edl, reinterpret_cast<uint32_t*>(rgba), index, depth_q);
    return sn::check_launch(what);
}
