// Shared by conv_i8s.hip (the int8 kernels) and bank.hip (the GENEO bank builder): the folded operand plan of a 9 x 9 x 9
// bank that is symmetric in x and y, and the per-bank preparation of the int8 contraction -- symmetry verdict, 24-bit
// fixed-point weights, worst-case quantisation error, digit table of the z-walk plan -- written into the caller-owned
// blob of sn_conv_bank_prep / sn_geneo_bank_prep (include/scenenet_hip.h).  Included INSIDE each translation unit's
// anonymous namespace (device code only; nothing here has linkage).
//
// Reference: SceneNet.forward rebuilds its kernels from the parameters at every call (core/models/SCENE_Net.py:322-327);
// everything below is a function of those weights alone.
#pragma once

constexpr double kQMax = 8355711.0;   // 127 * 65793: the largest magnitude three balanced base-256 digits hold

// The folded kernels' operand plan: kFoldSteps MFMA steps of kFoldRows folded kernel rows (dz, dx' <= 4) per lane group;
// slot (st, j) is SINGLE (dx' = 4: one halo row) for j = 2 of steps 0..2 and DOUBLE (halo rows dx' and 8 - dx' summed)
// elsewhere.  Regular slots: lane group q carries planes dz = 2 q + a.
constexpr int kFoldSteps = 4, kFoldRows = 3, kFoldSlots = kFoldSteps * kFoldRows;
constexpr bool fold_slot_single(int st, int j) { return j == 2 && st < 3; }
constexpr int fold_slot_a(int slot) { return slot >= 5 && slot != 8 && slot != 11 ? 1 : 0; }   // slots 0..4: a = 0; 5, 6, 7, 9, 10: a = 1
constexpr int fold_slot_dx(int slot) {
    return slot == 2 || slot == 5 ? 4 : slot == 0 || slot == 6 ? 0 : slot == 1 || slot == 7 ? 1 : slot == 3 || slot == 9 ? 2 : 3;
}
constexpr bool fold_slot_irregular(int slot) { return slot == 8 || slot == 11; }

// the preparation blob (caller-owned device memory, SN_CONV_PREP_BYTES per group of 16 kernels)
constexpr int kPrepWd = 0;                     // uint4 [4][3][64]   folded digit table of the z-walk plan
constexpr int kPrepScale = 12288;              // float [16]         max|W_g| / 8355711
constexpr int kPrepBnd = 12352;                // double [16]        worst-case quantisation error per kernel
constexpr int kPrepSym = 12480;                // int [16]           1: kernel g is bit-for-bit symmetric in x and y
constexpr int kPrepFit = 12544;                // int [16]           1: every partial digit recombination fits int32
constexpr int kPrepMagic = 12608;              // int                0x5a57414c once written
constexpr int kPrepZero = 12800;               // 16 zero bytes (the z-walk's LDS-DMA source for pieces outside the grid)
constexpr int kPrepRoute = 12672;              // int                the caller-owned route flag of the launches using this blob
                                               //                    (-1 fresh from the preparation; 0 / 1 / 2 a walk's verdict)
static_assert(kPrepRoute + 4 <= kPrepZero && kPrepZero + 16 <= SN_CONV_PREP_BYTES && kPrepZero % 16 == 0, "blob layout");

// slot -> folded kernel row of lane group qq (the z-walk plan; regular slots as FoldPlan: planes dz = 2 qq + a)
__host__ __device__ constexpr int zplan_krow(int qq, int slot) {
    if (slot == 8) return qq == 0 ? 8 * 9 + 4 : -1;       // the single of plane 8; pads elsewhere
    if (slot == 11) return 8 * 9 + qq;                    // plane 8's doubles: dx' = qq (rows one apart for the lane
                                                          // groups an LDS cycle serves: 16 banks in Yc)
    return (2 * qq + fold_slot_a(slot)) * 9 + fold_slot_dx(slot);
}

// ---- the folded quantiser, in pieces.  Every consumer -- the half-wave form inside the folded / z-walk kernels
// (quantise_folded_half) and the workgroup-wide form of the preparation (prep_one_kernel) -- is put together from these, so
// that all of them produce the same bits.
constexpr int kFoldUniq = 9 * 5 * 5;   // the unique taps of a kernel symmetric in x and y: u = (dz * 5 + dx) * 5 + dy, dx, dy <= 4

// unique tap u -> its tap index in the 9 x 9 x 9 kernel and the number of equal weights it stands for (the divisors are
// constants: multiply-shifts)
__device__ __forceinline__ int fold_tap(int u, int& mult) {
    const int r = (int)((unsigned)u / 5u), dy = u - 5 * r, dz = (int)((unsigned)r / 5u), dx = r - 5 * dz;
    mult = (dx < 4 ? 2 : 1) * (dy < 4 ? 2 : 1);
    return (dz * 9 + dx) * 9 + dy;
}

// one step of a lane's running maximum of |w| (an infinite or NaN weight poisons it)
__device__ __forceinline__ float fold_max_step(float m, float a) {
    return (a <= 3.0e38f) ? fmaxf(m, a) : __int_as_float(0x7fc00000);
}

// the 16 -> 1 butterfly of the maxima over a half wave
__device__ __forceinline__ float fold_max_half(float m) {
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) {
        const float u = __shfl_xor(m, o, 64);
        m = (m != m || u != u) ? __int_as_float(0x7fc00000) : fmaxf(m, u);
    }
    return m;
}

// one tap of a kernel whose maximum m is > 0: the fixed-point weight Q and its signed error term (times the multiplicity)
__device__ __forceinline__ void fold_quantise_tap(float wf, float m, int mult, int& Q, double& e) {
    const double S = kQMax / (double)m;
    const double invS = (double)m / kQMax;
    const double wv = (double)wf;
    Q = __double2int_rn(wv * S);
    e = ((double)Q * invS - wv) * (double)mult;
}

// a lane's running sums take one tap's terms (qm = Q * mult: exact, |Q| < 2^23)
__device__ __forceinline__ void fold_sums_step(double e, int qm, double& ep, double& en, double& qp, double& qn) {
    ep += e > 0.0 ? e : 0.0;
    en += e < 0.0 ? -e : 0.0;
    qp += qm > 0 ? (double)qm : 0.0;
    qn += qm < 0 ? -(double)qm : 0.0;
}

// the 16 -> 1 butterflies of the four sums, and what the blob takes from them
__device__ __forceinline__ void fold_sums_half(float m, double ep, double en, double qp, double qn, float& scale_out,
                                               double& bnd_out, double& pos_out, double& neg_out) {
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) {
        ep += __shfl_xor(ep, o, 64);
        en += __shfl_xor(en, o, 64);
        qp += __shfl_xor(qp, o, 64);
        qn += __shfl_xor(qn, o, 64);
    }
    scale_out = (m != m) ? m : (float)((double)m / kQMax);
    bnd_out = ep > en ? ep : en;
    pos_out = qp;
    neg_out = qn;
}

// one kernel's part of quantise_kernels_folded on the 32 lanes of a half wave (l32): `w` = the kernel's 729 fp32 weights in
// LDS (overwritten by Q at the unique taps); lane l32 takes the taps u = l32 + 32 k, k ascending
__device__ __forceinline__ void quantise_folded_half(float* w, bool valid, int l32, float& scale_out, double& bnd_out,
                                                     double& pos_out, double& neg_out) {
    float m = 0.0f;
    if (valid)
        for (int u = l32; u < kFoldUniq; u += 32) {
            int mult;
            m = fold_max_step(m, fabsf(w[fold_tap(u, mult)]));
        }
    m = fold_max_half(m);
    double ep = 0.0, en = 0.0, qp = 0.0, qn = 0.0;
    if (valid)
        for (int u = l32; u < kFoldUniq; u += 32) {
            int mult;
            const int t = fold_tap(u, mult);
            if (m > 0.0f) {
                int Q;
                double e;
                fold_quantise_tap(w[t], m, mult, Q, e);
                fold_sums_step(e, Q * mult, ep, en, qp, qn);
                w[t] = __int_as_float(Q);
            } else {
                w[t] = 0.0f;   // all-zero or poisoned kernel: Q = 0 (scale carries a NaN)
            }
        }
    fold_sums_half(m, ep, en, qp, qn, scale_out, bnd_out, pos_out, neg_out);
}


// The preparation of ONE kernel g by a workgroup of `nthreads` threads (a multiple of 64; all of them call; contains barriers):
// w = the kernel's 729 fp32 weights in LDS (zeros when !valid; overwritten -- the caller's writes to it need no barrier of
// their own), scr = kPrepScratchWords words of LDS, 16-byte aligned.  Symmetry verdict bitwise on the fp32 weights,
// quantisation and error bound with the folded kernel's own arithmetic (the pieces above), digit entries of the z-walk plan
// for lane (qq, g) of every step.  Every phase is one trip for a workgroup of 1024 threads: one tap, one term, one digit
// entry per thread.  What has an order keeps quantise_folded_half's: the 32 lanes of a half wave take the staged values of
// u = l32 + 32 k, k ascending, then the butterflies.
constexpr int kPrepScrE = 4, kPrepScrA = kPrepScrE + 512, kPrepScrQ = kPrepScrA + 256, kPrepScrDig = kPrepScrQ + 256;
constexpr int kPrepScratchWords = kPrepScrDig + 16 * 3 * 4;
static_assert(kFoldUniq <= 256 && kPrepScrDig % 4 == 0, "staging arrays of 256 entries; the digit rows are read as uint4");
// SN_BT(k): per-phase clocks of the body where it rides in a voxelisation launch.  voxel.hip defines it under SN_CONV_TIMING
// before it includes this file (clock k of the workgroup's row of g_vox_t, indexed by the host launch's own grid: rows of
// workgroups that a launch does not have keep an earlier launch's values -- tools/vox_timing.py reads the rows it knows);
// everywhere else it is nothing.
#ifndef SN_BT
#define SN_BT(k) do {} while (0)
#endif
// Threads per workgroup of the stand-alone kernels (sn_geneo_bank*, sn_conv_bank_prep): a multiple of 64, up to 1024.  These
// kernels are 16 workgroups on an idle device: 1024 measured 0.7 - 1.4 us faster for the bank kernels and no faster for the
// preparation, in one run each -- kept at the parent's 256 until that is repeated; the riders
// take their host kernel's workgroup instead.
#ifndef SN_BANK_THREADS
#define SN_BANK_THREADS 256
#endif
static_assert(SN_BANK_THREADS % 64 == 0 && SN_BANK_THREADS >= 64 && SN_BANK_THREADS <= 1024, "whole waves, one workgroup");

__device__ __forceinline__ void prep_one_kernel(float* w, float* scr, bool valid, int g, uint8_t* __restrict__ prep,
                                                int tid, int nthreads) {
    int* asym_s = reinterpret_cast<int*>(scr);
    double* e_s = reinterpret_cast<double*>(scr + kPrepScrE);   // [256] signed error term of unique tap u (0 beyond the 225)
    float* a_s = scr + kPrepScrA;                               // [256] |w| of unique tap u
    int* qm_s = reinterpret_cast<int*>(scr + kPrepScrQ);        // [256] Q x multiplicity of unique tap u
    uint8_t* dig_s = reinterpret_cast<uint8_t*>(scr + kPrepScrDig);   // [16 (st, qq)][3 digits][16 bytes (j, b)]
    const int lane = tid & 63, l32 = tid & 31;
    if (tid == 0) *asym_s = 0;
    __syncthreads();
    {   // the verdict: every tap against its mirror in x and its mirror in y; and |w| of the unique taps
        const uint32_t* wb = reinterpret_cast<const uint32_t*>(w);
        bool asym = false;
        for (int t = tid; t < 729; t += nthreads) {
            const int r = (int)((unsigned)t / 9u), dy = t - 9 * r, dz = (int)((unsigned)r / 9u), dx = r - 9 * dz;
            const uint32_t v = wb[t];
            asym |= (v != wb[(dz * 9 + 8 - dx) * 9 + dy]) | (v != wb[r * 9 + 8 - dy]);
        }
        if (asym) *asym_s = 1;
        for (int u = tid; u < kFoldUniq; u += nthreads) {
            int mult;
            a_s[u] = fabsf(w[fold_tap(u, mult)]);
        }
    }
    __syncthreads();
    SN_BT(4);
    // the maximum: lanes 0..31 of EVERY wave run the half wave's chain on the staged values (the same bits in each: no
    // broadcast through LDS, no barrier)
    float m = 0.0f;
    if (valid && lane < 32)
        for (int u = l32; u < kFoldUniq; u += 32) m = fold_max_step(m, a_s[u]);
    m = __shfl(fold_max_half(m), 0, 64);
    for (int u = tid; u < 256; u += nthreads) {
        double e = 0.0;
        int qm = 0;
        if (valid && u < kFoldUniq) {
            int mult;
            const int t = fold_tap(u, mult);
            if (m > 0.0f) {
                int Q;
                fold_quantise_tap(w[t], m, mult, Q, e);
                qm = Q * mult;
                w[t] = __int_as_float(Q);
            } else {
                w[t] = 0.0f;   // all-zero or poisoned kernel: Q = 0 (scale carries a NaN)
            }
        }
        e_s[u] = e;
        qm_s[u] = qm;
    }
    __syncthreads();
    SN_BT(5);
    for (int i = tid; i < 256; i += nthreads) {   // digit entry (st, qq, j, b); (j, b) = (3, 3) is a pad byte
        const int row = i >> 4, st = row >> 2, qq = row & 3, j = (i >> 2) & 3, b = i & 3;
        int d0 = 0, d1 = 0, d2 = 0;
        if (!(j == 3 && b == 3)) {
            const int slot = st * kFoldRows + (j < 3 ? j : b);
            const int krow = zplan_krow(qq, slot);
            const int dy = j < 3 ? b : 4;
            int Q = __float_as_int(w[(krow < 0 ? 0 : krow) * 9 + dy]);
            Q = (krow < 0 || !valid) ? 0 : Q;
            d0 = ((Q + 128) & 255) - 128;
            Q = (Q - d0) >> 8;
            d1 = ((Q + 128) & 255) - 128;
            d2 = (Q - d1) >> 8;
        }
        dig_s[(row * 3 + 0) * 16 + (i & 15)] = (uint8_t)(d0 & 255);
        dig_s[(row * 3 + 1) * 16 + (i & 15)] = (uint8_t)(d1 & 255);
        dig_s[(row * 3 + 2) * 16 + (i & 15)] = (uint8_t)(d2 & 255);
    }
    float sc = 0.0f;
    double bd = 0.0, qp = 0.0, qn = 0.0;
    if (tid < 64) {   // lanes 0..31 carry the kernel: the eight staged terms in k order from +0.0 (zero terms leave the bits alone)
        double ep = 0.0, en = 0.0, sp = 0.0, sm = 0.0;
        if (lane < 32)
#pragma unroll
            for (int k = 0; k < 8; ++k) fold_sums_step(e_s[l32 + 32 * k], qm_s[l32 + 32 * k], ep, en, sp, sm);
        fold_sums_half(m, ep, en, sp, sm, sc, bd, qp, qn);
    }
    __syncthreads();
    SN_BT(6);
    if (tid < 48) {
        const int row = tid / 3, d = tid - 3 * row, st = row >> 2, qq = row & 3;
        uint4* Wd = reinterpret_cast<uint4*>(prep + kPrepWd);
        Wd[(st * 3 + d) * 64 + qq * 16 + g] = reinterpret_cast<const uint4*>(dig_s)[tid];
    }
    if (tid == 0) {
        reinterpret_cast<float*>(prep + kPrepScale)[g] = sc;
        reinterpret_cast<double*>(prep + kPrepBnd)[g] = bd;
        reinterpret_cast<int*>(prep + kPrepSym)[g] = *asym_s ? 0 : 1;
        // |sum of any subset of the 729 signed weights x {0,1}| stays below 2^31: the digit sums may be recombined in int32
        reinterpret_cast<int*>(prep + kPrepFit)[g] = (qp < 2147483000.0 && qn < 2147483000.0) ? 1 : 0;
        if (g == 0) {
            *reinterpret_cast<int*>(prep + kPrepMagic) = 0x5a57414c;
            *reinterpret_cast<uint4*>(prep + kPrepZero) = make_uint4(0u, 0u, 0u, 0u);
            // the verdict word starts every preparation as "no walk has decided on THIS bank yet" (-1): a caller that learns
            // verdicts by reading the word back (PreparedVerdict) can then never take the previous bank's 0 -- or the zero a
            // fresh buffer holds -- for this bank's, e.g. after a call whose shape the walk does not serve
            *reinterpret_cast<int*>(prep + kPrepRoute) = -1;
        }
    }
    SN_BT(7);
}
