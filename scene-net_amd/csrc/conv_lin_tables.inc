// K3L's per-bank work as device code of its own, used by conv_lin.hip twice: by the kernel itself (every workgroup builds the
// tables in its LDS) and by the stand-alone preparation (one workgroup writes them into a caller-owned blob).  Included inside
// the includer's anonymous namespace.  (A rider form -- the tables built by one more workgroup of the voxelisation's launch,
// behind K2's bank -- is not built: K* needs ALL kernels of the bank, i.e. a hand-over between the riders.)
constexpr int kLinThreads = 512;
constexpr int kLinWaves = kLinThreads / 64;
constexpr int kLinTZ = 8, kLinTX = 16, kLinTY = 64;  // workgroup tile: one z plane per wave, 16 rows (N), 4 strips of 16 y (M)
constexpr int kLinYB = 80;                  // halo bytes per row (64 + 16) = 5 chunks of 16 bytes
// The halo is stored CHUNK-MAJOR, [chunk c][row r] x 16 bytes with the rows padded to a multiple of 16: the 16 lanes
// one ds_read_b128 cycle serves (8 with a window's first chunk, 8 with its second) then fall on 16 distinct 16-byte
// bank groups.
constexpr int kLinRowsPerPass = kLinThreads / (kLinYB / 4);   // halo rows one pass of the workgroup loads: a dword per thread
constexpr int kLinMaxLds = 160 * 1024;

struct LinShape {
    int B, Z, X, Y, G;
    int kz, kx, ky, pz, px, py;
    int nzt, nxt, nyt, ntiles;
    int npairs, nsteps;   // kernel rows (dz,dx); MFMA steps = ceil(npairs / 2)
    int XP, rows, NRP;    // halo rows per z plane, total halo rows, rows padded to a multiple of 16
    int PYA;              // halo origin in y = y0 - PYA, PYA = roundup(py, 4) (aligned global dwords)
    sn::Gate gate;       // run only if every condition holds (common.h: Gate)
    int32_t* route;       // out: 1 = K*'s quantisation bound exceeded (the gated fp32 launches behind take over), else 0
    float tol;            // bound on the worst-case pre-activation error allowed here (<= 0: no check)
    int dbg;              // timing experiments (SN_CONV_LIN_DBG): 1 prologue only, 2 no MFMA loop, 4 no epilogue, 16 no deferral
    const uint8_t* prep;  // tables prepared elsewhere (sn_conv_fused_prep): copied (LDS-DMA), not built
    int served;           // the caller left the gated fp32 launches out (assume_served): a kernel whose guard declines must
                          // not return quietly -- it fills `out` with NaN and latches the sticky status (common.h, code 2)
    int32_t* sticky;      // the device's sticky status words
};

// The prepared tables of one (bank, coefficients, kernel extent, tolerance): [At | offtab | scale, verdict]
struct LinBlob {
    size_t at_bytes, tab_off, tab_bytes, tail_off, bytes;   // tail: float scale, int32 verdict (1: quantisation bound exceeded)
};
__host__ __device__ inline LinBlob lin_blob_layout(int nsteps, bool w24) {
    LinBlob b;
    b.at_bytes = (size_t)(nsteps + 1) * 3 * 64 * 16;
    b.tab_off = b.at_bytes;
    b.tab_bytes = w24 ? (size_t)(nsteps + 3) * 8 * 4 : 0;
    b.tail_off = (b.tab_off + b.tab_bytes + 15) & ~(size_t)15;
    b.bytes = b.tail_off + 16;
    return b;
}


// K* = sum_g lambda_g K_g, its 24-bit fixed point, the worst-case quantisation error and the Toeplitz digit table (+ the
// 24-byte packing's offset table): the per-(bank, coefficients) work of K3L, by one workgroup of kLinThreads threads.
// At / offtab / scale_dst: where the tables go -- the kernel's own LDS (conv_lin_i8_kernel without a blob), or a blob in
// global memory (conv_lin_prep_kernel).  misc: 64 floats of LDS
// scratch, kstar: LDS scratch for K* and the padded digit rows.  Returns true when the bound exceeds s.tol (then the tables
// are not written); `publish`: this workgroup writes the verdict to `route`.
template <bool kW24>
__device__ __forceinline__ bool lin_tables(const float* __restrict__ bank, const float* __restrict__ lambdas, const LinShape& s,
                                           uint4* At, int* offtab, float* scale_dst, float* misc, float* kstar,
                                           int32_t* route, bool publish) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ntaps = s.kz * s.kx * s.ky;
    bool exceeded = false;
    // ---- prologue: K* = sum_g lambda_g K_g, its 24-bit fixed point, the Toeplitz digit table
    float mx = 0.0f;
    float w0[16], w1[16], l[16];
    auto kload = [&](int t0, int g0) {   // two taps x 16 kernels: 32 bank loads (+ the lambdas) in flight, one latency
        const int t1 = t0 + kLinThreads;
        const int t0c = t0 < ntaps ? t0 : 0, t1c = t1 < ntaps ? t1 : t0c;
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const int g = g0 + u < s.G ? g0 + u : s.G - 1;
            w0[u] = bank[(size_t)g * ntaps + t0c];
            w1[u] = bank[(size_t)g * ntaps + t1c];
            l[u] = g0 + u < s.G ? lambdas[g] : 0.0f;
        }
    };
    for (int t0 = tid; t0 < ntaps; t0 += 2 * kLinThreads) {
        const int t1 = t0 + kLinThreads;
        float a0 = 0.0f, a1 = 0.0f;
        for (int g0 = 0; g0 < s.G; g0 += 16) {   // the fp32 chain in kernel order
            kload(t0, g0);
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                a0 = fmaf(l[u], w0[u], a0);
                a1 = fmaf(l[u], w1[u], a1);
            }
        }
        kstar[t0] = a0;
        if (t1 < ntaps) kstar[t1] = a1;
        const float aa0 = fabsf(a0), aa1 = (t1 < ntaps) ? fabsf(a1) : 0.0f;
        mx = (aa0 <= 3.0e38f) ? fmaxf(mx, aa0) : __int_as_float(0x7fc00000);  // NaN / inf poisons the kernel
        mx = (aa1 <= 3.0e38f) ? fmaxf(mx, aa1) : __int_as_float(0x7fc00000);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float u = __shfl_xor(mx, o, 64);
        mx = (mx != mx || u != u) ? __int_as_float(0x7fc00000) : fmaxf(mx, u);
    }
    float* wmax = misc + 4;  // no static __shared__: the kernel asks for the whole 160 KiB dynamically
    if (lane == 0) wmax[wave] = mx;
    __syncthreads();
    // 24-bit fixed point over the whole range of three balanced digits: Q = rint(K* . S) in fp64, S = 8355711 / max|K*|
    double S = 0.0, invS = 0.0;
    {
        float m = 0.0f;
        for (int w = 0; w < kLinWaves; ++w) m = (m != m || wmax[w] != wmax[w]) ? __int_as_float(0x7fc00000) : fmaxf(m, wmax[w]);
        if (m > 0.0f) { S = 8355711.0 / (double)m; invS = (double)m / 8355711.0; }   // NaN: comparison false, S = 0 and the scale below is NaN
        if (tid == 0) misc[0] = (m != m) ? m : (float)((double)m / 8355711.0);   // (the scale; copied to *scale_dst below)
    }
    SN_LTT(5);   // (timing builds: K* and its maximum are done)
    double ep = 0.0, en = 0.0;   // this thread's share of the positive / negative quantisation errors
    // Each (kernel row p, digit d) as a zero-padded byte row R[64] with tap dy at byte 32 + dy; a table entry is the
    // 16-byte window of that row starting at byte 32 + 16 h - m - delta: five aligned dwords and four v_alignbyte
    // instead of quantising sixteen taps per entry (the table build was ~4 us of the prologue).
    constexpr int RW = 17;   // dwords per padded row (64 bytes + 1 zero dword for the look-ahead of the funnel shift)
    uint32_t* rpad = reinterpret_cast<uint32_t*>(kstar + ((ntaps + 3) & ~3));   // [npairs][3][RW]
    for (int i = tid; i < s.npairs * 3 * RW; i += kLinThreads) rpad[i] = 0u;
    __syncthreads();
    const int ngrp = (s.ky + 3) >> 2;   // dwords that hold taps: bytes 32 .. 32 + ky
    for (int i = tid; i < s.npairs * ngrp; i += kLinThreads) {
        const int p = i / ngrp, gq = i - p * ngrp;
        uint32_t w0 = 0u, w1 = 0u, w2 = 0u;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int dy = 4 * gq + j;
            if (dy < s.ky) {
                const double wv = (double)kstar[p * s.ky + dy];
                int Q = __double2int_rn(wv * S);
                if (S > 0.0) {
                    const double e = (double)Q * invS - wv;
                    ep += e > 0.0 ? e : 0.0;
                    en += e < 0.0 ? -e : 0.0;
                }
                const int d0 = ((Q + 128) & 255) - 128;
                Q = (Q - d0) >> 8;
                const int d1 = ((Q + 128) & 255) - 128;
                const int d2 = (Q - d1) >> 8;
                w0 |= (uint32_t)(d0 & 255) << (8 * j);
                w1 |= (uint32_t)(d1 & 255) << (8 * j);
                w2 |= (uint32_t)(d2 & 255) << (8 * j);
            }
        }
        rpad[(p * 3 + 0) * RW + 8 + gq] = w0;
        rpad[(p * 3 + 1) * RW + 8 + gq] = w1;
        rpad[(p * 3 + 2) * RW + 8 + gq] = w2;
    }
    // the exact worst case of the quantisation error over all binary inputs: max(sum of the positive errors, sum of the
    // negative ones).  Above the tolerance the launch is not run here: *route = 1 hands it to the fp32 contraction.
    double* esum = reinterpret_cast<double*>(misc + 16);   // [kLinWaves][2]
    if (s.tol > 0.0f) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            ep += __shfl_xor(ep, o, 64);
            en += __shfl_xor(en, o, 64);
        }
        if (lane == 0) { esum[2 * wave] = ep; esum[2 * wave + 1] = en; }
    }
    __syncthreads();
    if (s.tol > 0.0f) {
        double tp = 0.0, tn = 0.0;
        for (int w = 0; w < kLinWaves; ++w) { tp += esum[2 * w]; tn += esum[2 * w + 1]; }
        exceeded = (tp > tn ? tp : tn) > (double)s.tol;
        if (publish && tid == 0 && route) *route = exceeded ? 1 : 0;
        if (exceeded) return true;   // (uniform: every thread sums the same numbers)
    } else if (publish && tid == 0 && route) {
        *route = 0;
    }
    SN_LTT(6);   // (the padded digit rows and the error bound are done: what follows is the Toeplitz expansion)
    for (int i = tid; i < (s.nsteps + 1) * 64; i += kLinThreads) {
        const int st = i >> 6, l = i & 63;
        const int m = l & 15, qq = l >> 4;
        if constexpr (kW24) {
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                uint32_t o[4] = {0u, 0u, 0u, 0u};
#pragma unroll
                for (int e = 0; e < 2; ++e) {   // piece pi: window bytes 8 t .. 8 t + 7 of kernel row p
                    const int pi = 8 * st + 2 * qq + e;
                    const int p = pi / 3, t = pi - 3 * p;
                    if (p < s.npairs) {
                        const int s0 = 32 + 8 * t - m - (s.PYA - s.py);   // 14 .. 48
                        const uint32_t* r = rpad + (p * 3 + d) * RW + (s0 >> 2);
                        const uint32_t v0 = r[0], v1 = r[1], v2 = r[2];
                        o[2 * e] = __builtin_amdgcn_alignbyte(v1, v0, s0 & 3);
                        o[2 * e + 1] = __builtin_amdgcn_alignbyte(v2, v1, s0 & 3);
                    }
                }
                At[(st * 3 + d) * 64 + l] = make_uint4(o[0], o[1], o[2], o[3]);
            }
        } else {
            const int p = 2 * st + (qq >> 1);
            const int s0 = 32 + 16 * (qq & 1) - m - (s.PYA - s.py);   // first byte of this lane's window (14 .. 48)
            const int wq = s0 >> 2, sh = s0 & 3;
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                uint32_t o[4] = {0u, 0u, 0u, 0u};
                if (p < s.npairs) {
                    const uint32_t* r = rpad + (p * 3 + d) * RW + wq;
                    uint32_t v[5];
#pragma unroll
                    for (int j = 0; j < 5; ++j) v[j] = r[j];
#pragma unroll
                    for (int j = 0; j < 4; ++j) o[j] = __builtin_amdgcn_alignbyte(v[j + 1], v[j], sh);
                }
                At[(st * 3 + d) * 64 + l] = make_uint4(o[0], o[1], o[2], o[3]);
            }
        }
    }
    if constexpr (kW24) {   // piece -> halo byte offset (row (dz, dx), chunk t >> 1, half t & 1); past the end: 0
        for (int pi = tid; pi < (s.nsteps + 3) * 8; pi += kLinThreads) {
            const int p = pi / 3, t = pi - 3 * p;
            int off = 0;
            if (p < s.npairs) {
                const int dz = p / s.kx, dx = p - dz * s.kx;
                off = ((t >> 1) * s.NRP + dz * s.XP + dx) * 16 + 8 * (t & 1);
            }
            offtab[pi] = off;
        }
    }
    if (tid == 0) *scale_dst = misc[0];
    return false;
}

// The walk's two decisions outside the shape plan, each taken in ONE place: the kernel and the plan query
// (sn_conv_fused_plan) ask lin_defers, the launch and the query ask lin_grid.
// lin_defers: a tile's outputs ride along the first 16 MFMA steps of the workgroup's next tile -- needs that many steps.
__host__ __device__ inline bool lin_defers(int nsteps) { return nsteps >= 16; }
// lin_grid: persistent, one workgroup per compute unit (the LDS admits one), never more workgroups than tiles.
inline int lin_grid(int ntiles, int cus) { return cus < ntiles ? cus : ntiles; }

inline bool lin_plan(int B, int Z, int X, int Y, int G, int kz, int kx, int ky, LinShape& s, size_t& lds, bool& w24) {
    if (B <= 0 || Z <= 0 || X <= 0 || Y <= 0 || kz <= 0 || kx <= 0 || ky <= 0 || Y % 4 != 0) return false;
    s.B = B; s.Z = Z; s.X = X; s.Y = Y; s.G = G;
    s.kz = kz; s.kx = kx; s.ky = ky;
    s.served = 0; s.sticky = nullptr;   // (set by the launches that may be made with `assume_served`)
    s.pz = (kz - 1) / 2; s.px = (kx - 1) / 2; s.py = (ky - 1) / 2;
    s.PYA = (s.py + 3) & ~3;
    if (s.PYA - s.py + 15 + ky - 1 >= 32) return false;  // a 16-y strip's window must fit 32 halo bytes
    if (kLinTY - 16 + 32 > kLinYB) return false;
    s.nzt = (Z + kLinTZ - 1) / kLinTZ; s.nxt = (X + kLinTX - 1) / kLinTX; s.nyt = (Y + kLinTY - 1) / kLinTY;
    const long long nt = (long long)B * s.nzt * s.nxt * s.nyt;
    if (nt > 0x7fffffff) return false;
    s.ntiles = (int)nt;
    s.npairs = kz * kx;
    // 24-byte packing of the kernel rows when a strip's window fits 24 halo bytes (ky <= 9 with PYA == py)
    w24 = (s.PYA - s.py + 15 + ky - 1 < 24) && !sn::option(sn::kOptConvLinNo24);
    s.nsteps = w24 ? (3 * s.npairs + 7) / 8 : (s.npairs + 1) / 2;   // odd counts end with a lone step after the pairs
    s.XP = kLinTX + kx - 1;
    s.rows = (kLinTZ + kz - 1) * s.XP;
    s.NRP = (s.rows + 15) & ~15;
    const size_t halo = (size_t)s.NRP * kLinYB;
    // prologue scratch aliasing the halo: K* and the padded digit rows
    const size_t kst = (((size_t)kz * kx * ky + 3) & ~(size_t)3) * sizeof(float) + (size_t)kz * kx * 3 * 17 * 4;
    lds = (size_t)(s.nsteps + 1) * 3 * 64 * 16 + 256 + (w24 ? (size_t)(s.nsteps + 3) * 8 * 4 : 0) +
          (halo > kst ? halo : kst) + 16;
    return lds <= (size_t)kLinMaxLds;
}
