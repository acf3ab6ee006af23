// K9's regions -- the membership test of a disc / box row, the chunk-level reject and the chunk loaders -- shared by
// crops.hip (K9, K12) and scan_merge.hip (K19): one rule, one text.  Every file that includes this is built with
// -ffp-contract=off (Makefile): the disc test's products and sum are rounded once each.
#pragma once
#include "common.h"
#include "scan.h"

namespace {

using sn::kWaveLanes;     // scan.h: the chunk's geometry (kWaveGroups groups of 64 consecutive points held per lane) and
using sn::kWaveGroups;    // the prefix kernels' (kScanItems consecutive slots per thread and step)
using sn::kWaveChunk;
using sn::kScanThreads;
using sn::kScanItems;
using sn::readlane64;
constexpr int kMaxK = 1 << 16;
constexpr int64_t kMaxN = (int64_t)1 << 36;  // 2^26 workgroups

constexpr uint64_t kNaNBits = 0x7ff8000000000000ull;   // what a lane past the scan's end tests: in no region

struct Region {
    double a, b, c, d;   // disc: cx, cy, r*r, -;  box: xmin, ymin, xmax, ymax
    int kind;            // anything but SN_CROP_DISC / SN_CROP_BOX: empty
};

__device__ __forceinline__ double readlane_f64(double v, int j) {
    return __longlong_as_double((long long)readlane64((uint64_t)__double_as_longlong(v), j));
}

// row k of the table in the lane that asks for it; k >= K: an empty region
__device__ __forceinline__ Region load_region(const double* __restrict__ regions, const int32_t* __restrict__ kinds, int K,
                                              int k) {
    Region R{0.0, 0.0, 0.0, 0.0, -1};
    if (k < K) {
        const double* r = regions + (int64_t)k * 4;
        R.kind = kinds ? kinds[k] : (int)SN_CROP_DISC;
        R.a = r[0];
        R.b = r[1];
        R.c = R.kind == SN_CROP_DISC ? r[2] * r[2] : r[2];   // r*r: one rounding, |r| and r alike, NaN stays NaN
        R.d = r[3];
    }
    return R;
}
__device__ __forceinline__ Region broadcast(const Region& mine, int j) {
    Region R;
    R.a = readlane_f64(mine.a, j);
    R.b = readlane_f64(mine.b, j);
    R.c = readlane_f64(mine.c, j);
    R.d = readlane_f64(mine.d, j);
    R.kind = __builtin_amdgcn_readlane(mine.kind, j);
    return R;
}

// the membership test in exactly the documented form (R.kind is wave-uniform: a scalar branch)
__device__ __forceinline__ bool member(const Region& R, double x, double y) {
#pragma clang fp contract(off)
    if (R.kind == SN_CROP_DISC) {
        const double dx = x - R.a, dy = y - R.b;
        const double xx = dx * dx, yy = dy * dy;
        return xx + yy <= R.c;
    }
    if (R.kind == SN_CROP_BOX) return R.a <= x && x <= R.c && R.b <= y && y <= R.d;
    return false;
}

// Can no point of the xy box [xlo, xhi] x [ylo, yhi] be a member of R?  The box holds every point of the chunk whose x and y
// are not NaN (a NaN coordinate is a member of nothing), so lo <= x <= hi for every candidate.
// Box regions: a member has xmin <= x <= xmax, hence xhi >= x >= xmin and xlo <= x <= xmax (same for y): if one of the
// four fails there is no member.  A NaN bound makes its comparison false: no skip.
// Disc regions: the kernel's test is fl(fl(dx*dx) + fl(dy*dy)) <= R2 with dx = fl(x - cx), R2 = fl(r*r) -- the very R.c
// used here.  IEEE rounding is monotone, so (1) fl(a + b) >= a for a, b >= 0 (a is representable and a + b >= a): a member
// has fl(dx*dx) <= R2 and fl(dy*dy) <= R2;  (2) dx = fl(x - cx) is non-decreasing in x: dlo = fl(xlo - cx) <= dx <= dhi =
// fl(xhi - cx);  (3) fl(d*d) is non-decreasing in |d|.  If dlo > 0 every |dx| >= dlo, if dhi < 0 every |dx| >= |dhi|: with
// m that bound, fl(m*m) <= fl(dx*dx) <= R2 for a member, so fl(m*m) > R2 proves there is none.  The operations are the
// kernel's own, rounded the same way: no margin is needed, and a point a hair beyond |r| that the rounded test admits
// is admitted here as well.  NaN anywhere (centre, radius, inf - inf) makes the comparisons false: no skip.
__device__ __forceinline__ bool axis_out_of_reach(double lo, double hi, double c, double r2) {
    const double dlo = lo - c, dhi = hi - c;
    double m;
    if (dlo > 0.0) m = dlo;
    else if (dhi < 0.0) m = dhi;
    else return false;
    return m * m > r2;
}
__device__ __forceinline__ bool cannot_reach(const Region& R, double xlo, double xhi, double ylo, double yhi) {
    if (R.kind == SN_CROP_DISC) return axis_out_of_reach(xlo, xhi, R.a, R.c) || axis_out_of_reach(ylo, yhi, R.b, R.c);
    if (R.kind == SN_CROP_BOX) return xhi < R.a || xlo > R.c || yhi < R.b || ylo > R.d;
    return true;   // any other kind: empty
}

// smallest / largest of v over the wave, NaN left out (comparisons with a NaN are false); +inf / -inf if there is none
__device__ __forceinline__ void wave_min_max(const uint64_t (&bits)[kWaveGroups], double& lo, double& hi) {
    lo = __longlong_as_double(0x7ff0000000000000ll);
    hi = -lo;
#pragma unroll
    for (int g = 0; g < kWaveGroups; ++g) {
        const double v = __longlong_as_double((long long)bits[g]);
        lo = v < lo ? v : lo;
        hi = v > hi ? v : hi;
    }
    // (not two sn::wave_reduce: one after the other they schedule the count and census kernels differently)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double a = __shfl_xor(lo, off, 64), b = __shfl_xor(hi, off, 64);
        lo = a < lo ? a : lo;
        hi = b > hi ? b : hi;
    }
}

// x, y of the chunk's points as bit patterns; past the end: NaN
__device__ __forceinline__ void load_xy(const uint64_t* __restrict__ pts, int64_t n, int64_t base, int lane,
                                        uint64_t (&x)[kWaveGroups], uint64_t (&y)[kWaveGroups]) {
#pragma unroll
    for (int g = 0; g < kWaveGroups; ++g) {
        const int64_t i = base + g * kWaveLanes + lane;
        const bool in = i < n;
        x[g] = in ? pts[i * 3] : kNaNBits;
        y[g] = in ? pts[i * 3 + 1] : kNaNBits;
    }
}

}  // namespace
