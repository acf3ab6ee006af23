// Shared host-side helpers of the C ABI (error text, launch checks).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include "scenenet_hip.h"

namespace sn {

char* error_buffer();  // thread-local, 512 bytes (defined in cabi.hip)

inline int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(error_buffer(), 512, fmt, ap);
    va_end(ap);
    return code;
}

int sticky_check(const char* what);   // below / cabi.hip

inline int check_launch(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(SN_ERR_LAUNCH, "%s: %s", what, hipGetErrorString(e));
    return sticky_check(what);   // (a host read of pinned words; SN_OK unless a kernel has latched a status)
}

inline hipStream_t as_stream(sn_stream_t s) { return reinterpret_cast<hipStream_t>(s); }

// Process-wide runtime options (sn_set_option / sn_get_option): one entry each, in this order, in cabi.hip's option table
// (name, environment variable, default, range); include/scenenet_hip.h documents what each one does.
enum Opt {
    kOptConvSkipEmptyTiles,
    kOptConvI8TolerancePpb,
    kOptConvI8Fold,
    kOptConvI8Legacy,
    kOptConvI8NoStage,
    kOptConvI8zVariant,
    kOptConvNoI8,
    kOptConvDoubleBuffer,
    kOptConvLinNo24,
    kOptVoxelOnepass,
    kOptVoxelOnepassSpin,
    kOptCorrDense,
    kOptCorrSparseTileBytes,
    kOptConvI8zInjectFault,
    kOptConvI8zSegments,
    kOptConvI8zTrim,
    kOptConvI8zDense,
    kOptCount
};
// A relaxed atomic load.  An option with a variable reads it ONCE, at the first look (never per call: an environment
// lookup per launch sat on the production dispatch, and a stray variable could change kernels mid-run); an sn_set_option
// before that look wins.
int option(Opt which);   // cabi.hip
// the int8 kernels' quantisation guard compares its bound against exactly this float (0: guard off)
inline float conv_i8_tolerance() { return 1e-9f * (float)option(kOptConvI8TolerancePpb); }

// hipFuncAttributeMaxDynamicSharedMemorySize, set once per kernel (and raised when a launch needs more): the
// attribute call is not a stream operation, so steady-state launches stay free of it (cheaper, graph-capturable).
hipError_t ensure_dynamic_lds(const void* kernel, int bytes);  // cabi.hip

// Device-side gate of the conv launches made by this thread while a GateScope is alive: a kernel whose shape carries
// (gate, want) exits in its first instruction unless *gate == want (sn_forward_auto enqueues the int8 and the fp32
// form of the same forward and lets a device flag pick one -- no host synchronisation).
// Scopes nest (up to kGateDepth): every condition of the enclosing scopes must hold as well -- sn_forward_auto's
// "grid is binary" around the int8 kernels' "quantisation bound exceeded, run the fp32 form" (conv_i8s.hip).
constexpr int kGateDepth = 3;
struct Gate {
    const int32_t* ptr[kGateDepth];
    int want[kGateDepth];
    __device__ __forceinline__ bool pass() const {
#pragma unroll
        for (int i = 0; i < kGateDepth; ++i)
            if (ptr[i] && *ptr[i] != want[i]) return false;
        return true;
    }
};
Gate current_gate();          // all null outside a scope
struct GateScope {
    GateScope(const int32_t* ptr, int want);   // a fourth nested scope is a programming error: it aborts the process
    ~GateScope();
  private:
    int slot_;
};

// Debug bits of a kernel's shape: SN_DBG(shape, bit) is a COMPILE-TIME false in the product build -- no kernel carries
// a runtime test of a debug word; in a -DSN_CONV_DEBUG build it reads the shape's dbg field.
#ifdef SN_CONV_DEBUG
#define SN_DBG(shape, bit) (((shape).dbg & (bit)) != 0)
#else
#define SN_DBG(shape, bit) false
#endif
// Wrong-result timing switches (a skipped epilogue, idle waves ...) exist only in builds made with -DSN_CONV_DEBUG
// (make EXTRA=-DSN_CONV_DEBUG): in the product they read as 0 whatever the environment says.
inline int debug_env_int(const char* name) {
#ifdef SN_CONV_DEBUG
    const char* v = getenv(name);
    return v ? atoi(v) : 0;
#else
    (void)name;
    return 0;
#endif
}

// ---- sticky device status (round 4): a kernel that cannot keep its contract (a dependency spin that gave up, a launch
// made with `assume served` whose bank the guard declines) must not return plausible numbers.  It poisons what it owns
// (NaN) and LATCHES a status in four host-pinned words per device; every sn_* launch path looks at them (check_launch,
// a host memory read: no synchronisation) and fails with SN_ERR_DEVICE_STATUS until sn_device_status_clear().
//   words: [0] code (0: healthy)  [1] claim (first reporter wins)  [2], [3] detail (workgroup, ticket / verdict)
//   codes: 1 a dependency spin of the z-walk gave up;  2 a `served` launch of the z-walk declined its bank;
//          3 a tile kernel's (folded / stride-4 / four-copy) spin gave up
void take_timing_events(hipEvent_t& start, hipEvent_t& stop);   // cabi.hip: the pair set by sn_launch_timing_events, consumed
int32_t* sticky_device_ptr(hipStream_t stream);   // cabi.hip: the current device's words as a DEVICE pointer (nullptr: not allocated
                                                  // and `stream` is capturing -- nothing is ever allocated inside a capture)
int sticky_check(const char* what);   // cabi.hip: SN_OK, or SN_ERR_DEVICE_STATUS with the latched code in the error text
__device__ __forceinline__ void sticky_latch(int32_t* sticky, int code, int a, int b) {
    if (!sticky) return;
    // (a, b are wave-uniform; made opaque HERE so that hipcc does not materialise them in vector registers ahead of the hot
    // loop the latch sits behind -- [measured in the ISA] it hoisted a v_mov of blockIdx.x out of the z-walk's ticket loop and
    // spilled it: the kernel's only scratch use)
    a = __builtin_amdgcn_readfirstlane(a);   // (uniform by contract; the readfirstlane makes it so for the register allocator,
    b = __builtin_amdgcn_readfirstlane(b);   // whatever it thinks of the caller's expression)
    asm volatile("" : "+s"(a), "+s"(b));
    if (__hip_atomic_exchange(&sticky[1], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) == 0) {
        __hip_atomic_store(&sticky[2], a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(&sticky[3], b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(&sticky[0], code, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// Order-preserving map of an fp64 to a uint64 (a < b  <=>  enc(a) < enc(b) for values that are not NaN; -0.0 sorts below
// +0.0) and back: what lets integer atomicMin / atomicMax reduce fp64 minima and maxima (K1's boxes, K12's label range).
__device__ __forceinline__ unsigned long long enc_f64(double d) {
    unsigned long long u = (unsigned long long)__double_as_longlong(d);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double dec_f64(unsigned long long u) {
    u = (u >> 63) ? (u & 0x7fffffffffffffffull) : ~u;
    return __longlong_as_double((long long)u);
}

// f32 bit pattern -> the f64 bit pattern of the same value, by integer arithmetic only (exact for every finite value and
// infinity; a NaN keeps its sign and payload and gets the quiet bit, as an IEEE conversion gives), so the result does not
// depend on the floating-point mode: how K7's f32 rows and K14's velodyne floats are widened.
__device__ __forceinline__ uint64_t widen_f32_bits(uint32_t u) {
    const uint64_t sign = (uint64_t)(u >> 31) << 63;
    const uint32_t e = (u >> 23) & 0xffu, m = u & 0x7fffffu;
    if (e == 0xffu) return sign | 0x7ff0000000000000ull | ((uint64_t)m << 29) | (m ? 0x0008000000000000ull : 0ull);
    if (e == 0) {
        if (m == 0) return sign;
        const int p = 31 - __clz((int)m);   // m * 2^-149 = 1.f * 2^(p - 149), p in 0..22
        return sign | ((uint64_t)(p - 149 + 1023) << 52) | ((uint64_t)(m - (1u << p)) << (52 - p));
    }
    return sign | ((uint64_t)(e + (1023 - 127)) << 52) | ((uint64_t)m << 29);
}

// One int of device memory per call (the flag an int8 launch leaves for the gated fp32 launch enqueued behind it, dynamic
// tile tickets): from a recycled ring for eager launches, from a never-recycled pool while `stream` is capturing
// (cabi.hip).  nullptr if the pool cannot be allocated.
int32_t* device_flag_slot(hipStream_t stream);

}  // namespace sn
