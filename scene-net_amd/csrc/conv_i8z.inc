// K3'z -- the folded int8 contraction as a Z-WALK over PRE-FOLDED planes (included by conv_i8s.hip, inside its anonymous
// namespace: same Shape / finish_round / quantisation helpers, and the stride-4 body as the in-launch fallback).
//
// Same contraction, same integers and the same head as conv_occ_i8f_kernel (SceneNet.forward,
// core/models/SCENE_Net.py:322-339, on a bank that is symmetric in x and y: 9 x 5 x 5 folded taps, 4 MFMA steps per
// 16 x 16 outputs, three digit planes).  What differs is WHERE the folding is done and how a workgroup moves:
//
//   [measured, round 3, tools/fold_floor.sh] the folded kernel is bound by instruction issue, not by the matrix pipe:
//   with its MFMAs compiled out it takes as long (120.8 vs 119.2 us), without the y fold 99.4 us, without the epilogue
//   90.0 us, without both 75.0 us.  A round re-folds every operand from raw halo bytes (264 VALU of 570), although the
//   folded window of a halo row depends on (plane, row, lane) only and is consumed by up to nine rounds.
//
//   * a workgroup owns a COLUMN (tile b, 8 x-rows, 64 y) and walks z.  Input planes arrive once, as LDS-DMA of their 16
//     raw halo rows (96 B each); a FOLD PASS turns four rows at a time into their y-folded form -- per lane n and
//     residue r one dword  F[r] = bytes(r..r+3) + bytes(r+8..r+5)  (values 0..2) plus the centre dword -- and writes it
//     to a ring of 16 planes (Yq: 16 B per lane, 4 KB per plane; Yc: the centre dwords).  Every plane is fetched and
//     folded ONCE per column (the tile kernel fetched it ~2x and folded it up to 9x).
//   * a round (2 x-rows x 64 y x 16 kernels of one output plane z) reads its 24 operand units straight from the ring:
//     ds_read_b128 + ds_read_b32 per halo row, the x fold is 5 v_add per unit, the centres' byte transposes stay.
//     No y fold in the rounds: ~350 VALU per round instead of 570.
//   * no tiles, no barriers after the prologue: ONE ticket counter orders everything.  Ticket t = (slot s = t >> 2,
//     pass xr = t & 3) carries  (a) the LDS-DMA of four raw rows of plane s + 4,  (b) the fold pass of four rows of plane
//     s,  (c) round xr of the output plane whose nine input planes were folded at least two slots ago.  All hand-overs
//     are monotonic LDS counters per ring slot (landed / folded / read), checked with ONE LDS read per ticket; every
//     dependency points to an earlier ticket, so the walk cannot deadlock.  A spin that gives up is LOUD (round 4): the
//     workgroup stops, overwrites everything it owns in `out` / `act` with NaN and latches the device's sticky status
//     (sn_device_status; every later sn_* call on the device fails until it is cleared) -- it never leaves plausible
//     numbers computed from a stale ring slot.  What each hand-over rests on is written down where it happens (HAND-OVER
//     1..4 below), checked on the ISA of every shipped instantiation by tools/zwalk_handover_audit.py (CPU test), on the
//     protocol by tools/debug/zwalk_protocol_sim.py (hazard model, adversarial schedules; CPU test), and on the part by
//     tools/micro/ldsdma_handover.hip (profiles/r04_ldsdma_handover.txt: 1.2e9 hot hand-overs, no stale word).
//   * the per-bank work -- symmetry verdict, 24-bit quantisation, worst-case error bounds, digit table -- is NOT repeated
//     by 256 workgroups: a preparation kernel (sn_conv_bank_prep, or the tail of sn_geneo_bank_prep on K2's side
//     stream) writes it once into a caller-owned blob; the walk's prologue copies 12 KB.
//
// Ring arithmetic: plane u of the workgroup's plane stream (job k = u / PL, p = u % PL: grid plane zs_k - 4 + p) lives in
// slot u & 15 of both rings.  Output o of job k needs planes k PL + o .. + 8; its four rounds ride on slot
// k PL + o + kZD.  A fold pass at slot s overwrites plane s - 16, whose readers rode on slots s - 14 .. s - 6.  (The head-only
// form maps a stream position to its job with a cursor, and its jobs may differ in length: TRIMMED JOBS below.)
//
// EMPTY WINDOWS (round 6).  The input is LiDAR occupancy: a few per cent of the voxels are set, and a round whose operand
// window -- 9 planes x 9 halo rows x the column's 96 halo bytes in y -- holds no set voxel has twelve accumulators that are
// exactly 0.  The walk does not run such a round:
//   * the fold pass has row 4 xr + q of its plane in registers (lane (q, n): the three raw dwords R0 R1 R2, i.e. the y window
//     of that lane's four outputs +- 4).  A row is NON-EMPTY when (R0 | R1 | R2) != 0 in any of its 16 lanes: one ballot per
//     pass, four row bits (scalar: s_quadmask twice), written by one lane as BYTE xr of the dword rowmask[u & 15] (bit q of byte xr = row 4 xr + q; four
//     passes by four waves never read-modify-write each other).  The store goes out ahead of the pass's folded[] report.
//     The rule is CONSERVATIVE: a row's bit covers the whole y extent the 16 lanes read (y0 - 4 .. y0 + 67, clipped to the
//     grid), and the 16 rows x0 - 4 .. x0 + 11, halo included, so a voxel that only a neighbouring column's or y tile's
//     outputs need still sets it.  It never calls a window empty that is not.
//   * a ticket reads the nine mask dwords of its planes in ONE ds_read_b32 (lanes 0..8, the counter index its dependency
//     check formed) behind the check and ahead of its passes -- guarded like the ring: valid once folded[] of the nine slots
//     is complete, protected from the fold that reuses a slot by the read[] report (hand-over 3), which every path issues
//     behind a wait for the read's return (a ticket without a round reads too and drops the value).  A round of x-rows
//     h .. h + kH - 1 is empty when no lane's dword has one of the row bits h .. h + kH + 7.
//   * an empty round issues no operand read, no weight read and no MFMA; it stores what finish_round would store for
//     all-zero accumulators (zero_round: + 0.0 activations; for `out` the same operations from e = + 0.0 on: the head & 1
//     load-and-add, the head & 2 relu_tanh).  That equals the full epilogue bit for bit iff coefficient x 0 = + 0, so the
//     prologue allows skipping (can_skip, workgroup-uniform) only if all 16 entries of scale, lamsc and lamhi are finite
//     (scale not negative) and sn_set_option("conv_i8z_dense") is 0; otherwise every round runs, NaN / inf propagate.
//   sn_conv_i8z_round_counts: rounds run / skipped, summed per workgroup in LDS and added once at its end.
//
// THE LEAN TICKET (round 7, head-only form).  [measured, tools/micro/issue_model.hip s] a scalar instruction costs a SIMD 3.6
// cycles at three waves per SIMD (the CU's one scalar unit serves four SIMDs) and only part of the other waves' vector issue
// hides beside it; a ticket of round 6 whose two rounds were empty still executed ~325 scalar and ~135 vector instructions, and
// on an all-zero batch the part of a ticket behind its passes was 52 % of a wave's time.  So a ticket forms its verdict FIRST,
// from one union window over all its rounds (rows lx .. lx + kH kR + 7; the mask a constant selected by lx & 3 and shifted by
// bytes, not rebuilt with shifts and ors), and when that is empty it issues nothing of the round set-up: the read[] report
// (behind the wait for the mask read, as before), one scalar row address from the job's base out + b V -- formed when the job
// changes, as is x + b V for the LDS-DMA -- and the stores of the constant + 0.0 (relu_tanh(+ 0.0) is + 0.0: see relu_tanh),
// both rows in one store of two values per lane where they are contiguous (one y tile spans Y), else two stores from the one
// base; under head & 1 the load-add-activate of zero_round1 / zero_round2 stays.  The per-round verdicts, the table reads and
// the ring addresses are formed only for a ticket that runs a round.  The activations form (kAct) keeps the round-6 ticket:
// see kLean in the kernel.
//
// DEAD JOBS (round 8, head-only form).  The launch ends with its busiest columns.  Under the dealt plan (ZShape::deal, fill_dead:
// sn_set_option("conv_i8z_segments"), conv_i8s.hip) a column is cut into z segments that go to different workgroups, and a
// workgroup checks its own jobs in its prologue: one whose whole operand region holds no set voxel is not streamed at all -- its
// outputs are filled with what its rounds would have stored and its rounds counted as skipped -- and the ticket loop walks the
// live jobs only.  No extra launch, nothing shared between workgroups, nothing in the ticket loop: see DEAD JOBS in the kernel.
//
// TRIMMED JOBS (head-only form, where THE BALANCED DEAL stands; sn_set_option("conv_i8z_trim")).  A live job used to stream
// LZ + 8 planes whatever it held; a plane costs its four tickets (claim, dependency check, LDS-DMA, fold pass).  Output plane z
// of a job is LIVE when the nine-plane window W[z] of the tile's row bits has a bit in rows x0 - 4 .. x0 + 11; a plane that is
// not has every round empty under EMPTY WINDOWS' rule.  After the deal -- which does not change: same costs, same tables -- a
// live job is cut to [a, a + len): from its first to its last live output plane, never below min(8, LZ) outputs (the shortest
// uniform job the launch rules allow: 16 planes, one ring's worth), padded upwards, and downwards where the segment ends first.
// Job k of the workgroup's live jobs occupies stream positions [S_k, S_k + len_k + 8); its output o is grid plane a_k + o, its
// plane p grid plane a_k - 4 + p.  The hand-over protocol lives in stream coordinates and is untouched: only the map from a
// stream position to (job, plane) changes, from a division by PL to a CURSOR (a wave's positions only grow: it keeps its job's
// stream end and steps to the next job when a position reaches it -- one LDS read when the job changes, none otherwise).  The
// flanks [z0, a) and [a + len, z1) are filled in the prologue with the dead jobs, their rounds counted as skipped.
// sn_conv_i8z_plane_counts: planes streamed / trimmed away (head-only form), per workgroup in LDS, added once at its end.

constexpr int kZTX = 8;                        // output x-rows per column
constexpr int kZRows = kZTX + 8;               // halo rows per plane
constexpr int kZRing = 16;                     // planes in the raw ring and in the folded ring
#ifndef SN_I8Z_LAG
#define SN_I8Z_LAG 3   // [measured] C2: 2 -> 100.9 us, 3 -> 98.3, 4 -> 100.1 (a round waited 6 % of its wave's time for folds
                       // that tickets 5..8 places earlier -- with twelve waves, often still in flight -- had not finished)
#endif
constexpr int kZLag = SN_I8Z_LAG;              // a round starts this many slots after its newest plane's fold
constexpr int kZD = 8 + kZLag;                 // output stream position sigma rides on slot sigma + kZD
#ifndef SN_I8Z_DD
#define SN_I8Z_DD 4
#endif
constexpr int kZDD = SN_I8Z_DD;                // LDS-DMA runs this many planes ahead of the fold
constexpr int kZPre = kZD + kZDD;              // planes the prologue requests
constexpr int kZRawPlane = kZRows * DW * 4;    // 1536 B
constexpr int kZYqRow = 256, kZYqPlane = kZRows * kZYqRow;   // 16 lanes x 16 B; every row starts on bank 0: any two rows are
                                                             // bank-disjoint for the lane groups of a ds_read_b128
constexpr int kZYcRow = 64, kZYcPlane = kZRows * kZYcRow + 32;   // 264 dwords: planes 2 apart (lane groups 0/1, 2/3) and
                                                                 // planes -14 apart (ring wrap) are 16 banks apart (mod 32)
constexpr int kZMaxJobs = 256;                 // jobs per workgroup (job table in LDS)
// THE BALANCED DEAL: jobs per tile (one lane each), and a job's cost in nanoseconds of the plan model (DESIGN section 4:
// 0.52 us per plane streamed, 0.122 us per round run; a dead job is its fill, 16 KB .. 64 KB of stores)
constexpr int kZBalJobs = 64;
constexpr int kBalPlane = 520, kBalRound = 122, kBalFill = 300;
// Skip mode only: cut every column into this many z segments and deal segment sg of column xt to the workgroup of column
// xt + SN_I8Z_SKIP_SHIFT sg, so that a workgroup's work comes from several columns (0: the plan of the dense walk).
#ifndef SN_I8Z_SKIP_NSEG
#define SN_I8Z_SKIP_NSEG 0
#endif
#ifndef SN_I8Z_SKIP_SHIFT
#define SN_I8Z_SKIP_SHIFT 0
#endif
#ifndef SN_I8Z_AHEAD
#define SN_I8Z_AHEAD 2                         // operand units are requested this many pieces before their fold
#endif
static_assert(kZRing == 16 && (kZYcPlane / 4) % 16 == 8, "ring and bank arithmetic below");
static_assert(kZRing - 8 - kZLag >= 2, "the readers of a plane ride at least two slots before its overwrite");
static_assert(kZPre <= kZRing, "the prologue's planes fit the raw ring");

// (blob layout kPrep*, zplan_krow, prep_one_kernel: conv_prep.h)

struct ZJob {
    int b, x0, y0, zs;
};

struct ZShape {
    int B, Z, X, Y, G, Gtot, g0, head;
    int nxt, nyt, nseg, LZ, PL;   // columns = B x nxt x nyt, z segments per column, outputs / planes per job
    int njobs;                    // all workgroups together
    unsigned pl_magic;            // u / PL == mulhi(u, pl_magic) for every u the kernel forms (checked on the host)
    int swizzle;                  // jobs of one round of the grid are dealt XCD-major (x-adjacent columns share an L2)
    float tol;
    sn::Gate gate;
    int32_t* route;
    int served;                   // the caller left the fallback launch out (sn_conv_bank_prepared_served): a walk that declines
                                  // must not return quietly -- it poisons its outputs and latches the sticky status
    int fill_dead;                // head-only form, dealt plan: a workgroup drops the jobs whose operand region holds no set voxel
                                  // from its stream and fills their outputs in its prologue (DEAD JOBS).  (In what was padding:
                                  // no other field moves, the activations form's argument loads stay as they were.)
    int32_t* sticky;              // the device's sticky status words (host-pinned, cabi.hip: sn::sticky_device_ptr)
    int dbg;
    int dense;                    // sn_set_option("conv_i8z_dense"): run every round, whatever its window holds
    int deal, deal_shift;         // jobs in segment-major order, segment sg of column (b, yt, xt) dealt as column xt + shift sg
                                  // (mod nxt): a workgroup's segments come from different columns (SN_I8Z_SKIP_NSEG)
    int bal;                      // THE BALANCED DEAL: the workgroups of a tile share its jobs by cost, from `rows`
    int trim;                     // TRIMMED JOBS (bal only; sn_set_option("conv_i8z_trim")): a live job streams its live output
                                  // planes only
    const uint32_t* rows;         // the occupancy's row bits [B][Z][ceil(X / 32)] (sn_conv_bank_prepared_rows), bal only
    int32_t* plan_out;            // nullable, bal only: row blockIdx.x of [grid][1 + kZBalJobs] = (count, job numbers ...)
};

// diagnostics (sn_conv_i8z_round_counts): rounds the walk ran / skipped (empty operand window), all launches since load
__device__ unsigned long long g_zwalk_rounds[2] = {0ull, 0ull};
// ... (sn_conv_i8z_plane_counts): planes the head-only walk streamed / did not stream because TRIMMED JOBS cut them away
__device__ unsigned long long g_zwalk_planes[2] = {0ull, 0ull};

__device__ __forceinline__ int zjob_id(const ZShape& z, int wg, int k, int grid) {
    const int base = k * grid;
    if (z.swizzle && base + grid <= z.njobs) return base + (wg & 7) * (grid >> 3) + (wg >> 3);
    return base + wg;
}

// ------------------------------------------------------------------------------------------------ preparation kernel
// One workgroup per kernel g (always 16 workgroups: g >= G writes zero entries); the work itself is prep_one_kernel
// (conv_prep.h), which the GENEO bank builder also runs as its tail (sn_geneo_bank_prep).  ~3 us.
constexpr int kPrepThreads = SN_BANK_THREADS;   // (conv_prep.h)
__global__ __launch_bounds__(kPrepThreads) void conv_prep_kernel(const float* __restrict__ bank, int G,
                                                                 uint8_t* __restrict__ prep) {
    __shared__ __align__(16) float w[732 + kPrepScratchWords];
    const int g = blockIdx.x, tid = threadIdx.x;
    const bool valid = g < G;
    for (int i = tid; i < 729; i += kPrepThreads) w[i] = valid ? bank[(size_t)g * 729 + i] : 0.0f;
    prep_one_kernel(w, w + 732, valid, g, prep, tid, kPrepThreads);
}

// ------------------------------------------------------------------------------------------------------ the walk
// One round's epilogue for a round of ONE x-row (kH = 1: four accumulator tiles, the residues): the same operations in the
// same order as finish_round on those tiles -- the digit recombination, the bank activations, the head's mix as packed
// FMAs over tile pairs (0, 1) and (2, 3), the sum over the four lane groups as (q + q+2) then (even + odd) -- so a voxel's
// value has the same bits whichever kernel produced it.  Lane group q ends up holding residue q: one value per lane,
// 64 consecutive y per wave store.
// (col = 4 n + q and q16 = 16 q come from the walk's lane table: the head-only form needs nothing else of the lane id)
template <typename OT, typename SH>
__device__ __forceinline__ void finish_round1(const SH& s, const TileCoord& c, int lx, int n, int q, int col, int q16,
                                              i32x4 (&acc)[3][4], const float* scale, const float* lamsc, const float* lamhi,
                                              OT* __restrict__ act, OT* __restrict__ out, size_t V) {
    const int gz = c.z0;
    const int gx = c.x0 + lx;
    if (gz >= s.Z || gx >= s.X) return;
    const int gy4 = c.y0 + 4 * n;
    float pm[4];
    const float4 lam4 = *reinterpret_cast<const float4*>(reinterpret_cast<const uint8_t*>(lamsc) + q16);
    const float lam[4] = {lam4.x, lam4.y, lam4.z, lam4.w};
    if (act) {
        float val[4][4];
#pragma unroll
        for (int v = 0; v < 4; ++v)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int low = acc[1][v][r] * 256 + acc[0][v][r];
                val[v][r] = fmaf((float)acc[2][v][r], 65536.0f, (float)low);
            }
        const float4 sc4 = *reinterpret_cast<const float4*>(scale + 4 * q);
        const float sc[4] = {sc4.x, sc4.y, sc4.z, sc4.w};
        if (gy4 < s.Y) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int g = 4 * q + r;
                if (g < s.G) {
                    OT* o = act + ((size_t)c.b * s.Gtot + s.g0 + g) * V + ((size_t)gz * s.X + gx) * s.Y + gy4;
                    const float v0 = val[0][r] * sc[r], v1 = val[1][r] * sc[r], v2 = val[2][r] * sc[r], v3 = val[3][r] * sc[r];
                    if constexpr (sizeof(OT) == 4) {
                        *reinterpret_cast<float4*>(o) = make_float4(v0, v1, v2, v3);
                    } else {
                        reinterpret_cast<double2*>(o)[0] = make_double2((double)v0, (double)v1);
                        reinterpret_cast<double2*>(o)[1] = make_double2((double)v2, (double)v3);
                    }
                }
            }
        }
    }
    {
        // (packed FMAs, as finish_round: [measured] the same FMAs issued as scalar v_fma_f32 took 113.1 us against 107.4)
        using f32x2 = __attribute__((ext_vector_type(2))) float;
        const float4 hi4 = *reinterpret_cast<const float4*>(reinterpret_cast<const uint8_t*>(lamhi) + q16);
        const float lhi[4] = {hi4.x, hi4.y, hi4.z, hi4.w};
#pragma unroll
        for (int vp = 0; vp < 2; ++vp) {
            const int v0 = 2 * vp, v1 = 2 * vp + 1;
            f32x2 p = {0.0f, 0.0f};
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int low0 = acc[1][v0][r] * 256 + acc[0][v0][r], low1 = acc[1][v1][r] * 256 + acc[0][v1][r];
                const f32x2 lo = {(float)low0, (float)low1};
                const f32x2 hi = {(float)acc[2][v0][r], (float)acc[2][v1][r]};
                p = __builtin_elementwise_fma(f32x2{lam[r], lam[r]}, lo, p);
                p = __builtin_elementwise_fma(f32x2{lhi[r], lhi[r]}, hi, p);
            }
            pm[v0] = p.x;
            pm[v1] = p.y;
        }
    }
    if (out) {
        auto sum_halves = [&](float a, float b) -> float {
            const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(a), __float_as_uint(b), false, false);
            return __uint_as_float(r[0]) + __uint_as_float(r[1]);
        };
        auto sum_rows = [&](float u, float w) -> float {
            const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(u), __float_as_uint(w), false, false);
            return __uint_as_float(r[0]) + __uint_as_float(r[1]);
        };
        // lower half: tiles 0 / 1, upper half: tiles 2 / 3; then even lane groups keep the first, odd ones the second:
        // lane group q holds residue q
        const float e = sum_rows(sum_halves(pm[0], pm[2]), sum_halves(pm[1], pm[3]));
        const int gy = c.y0 + col;
        if (gy < s.Y) {
            OT* row = out + ((size_t)c.b * V + ((size_t)gz * s.X + gx) * s.Y + c.y0);
            OT* o = row + (unsigned)col;
            float t0 = e;
            if (s.head & 1) t0 += (float)load_now(o);
            if (s.head & 2) t0 = relu_tanh(t0);
            *o = (OT)t0;
        }
    }
}

// What finish_round1 / finish_round store for a round whose accumulators are all zero, when every coefficient is finite
// (can_skip): val = fma(0, 65536, 0) = + 0 and + 0 x scale = + 0 (scale >= 0); the packed FMAs give lam x 0 + (+ 0) = + 0
// whatever lam's sign, the lane sums + 0 + + 0 = + 0; from e = + 0 on the operations are the epilogue's own (the zero is made
// opaque so that they are issued, not folded).
template <typename OT>
__device__ __forceinline__ void zero_act_row(OT* o) {
    if constexpr (sizeof(OT) == 4) {
        *reinterpret_cast<float4*>(o) = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    } else {
        reinterpret_cast<double2*>(o)[0] = make_double2(0.0, 0.0);
        reinterpret_cast<double2*>(o)[1] = make_double2(0.0, 0.0);
    }
}
template <typename OT, typename SH>
__device__ __forceinline__ void zero_round1(const SH& s, const TileCoord& c, int lx, int n, int q, int col,
                                            OT* __restrict__ act, OT* __restrict__ out, size_t V) {
    const int gz = c.z0;
    const int gx = c.x0 + lx;
    if (gz >= s.Z || gx >= s.X) return;
    const int gy4 = c.y0 + 4 * n;
    if (act && gy4 < s.Y) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int g = 4 * q + r;
            if (g < s.G) zero_act_row(act + ((size_t)c.b * s.Gtot + s.g0 + g) * V + ((size_t)gz * s.X + gx) * s.Y + gy4);
        }
    }
    if (out) {
        const int gy = c.y0 + col;
        if (gy < s.Y) {
            OT* row = out + ((size_t)c.b * V + ((size_t)gz * s.X + gx) * s.Y + c.y0);
            OT* o = row + (unsigned)col;
            float t0 = 0.0f;
            asm volatile("" : "+v"(t0));
            if (s.head & 1) t0 += (float)load_now(o);
            if (s.head & 2) t0 = relu_tanh(t0);
            *o = (OT)t0;
        }
    }
}
// (two x-rows: finish_round's stores)
template <typename OT, typename SH>
__device__ __forceinline__ void zero_round2(const SH& s, const TileCoord& c, int lx, int n, int q, OT* __restrict__ act,
                                            OT* __restrict__ out, size_t V) {
    const int gz = c.z0;
    if (gz >= s.Z) return;
    const int gy4 = c.y0 + 4 * n;
    if (act && gy4 < s.Y) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int gx = c.x0 + lx + h;
            if (gx < s.X) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int g = 4 * q + r;
                    if (g < s.G) zero_act_row(act + ((size_t)c.b * s.Gtot + s.g0 + g) * V + ((size_t)gz * s.X + gx) * s.Y + gy4);
                }
            }
        }
    }
    if (out) {
        const int h = q >> 1;
        const int gx = c.x0 + lx + h, gy = gy4 + 2 * (q & 1);
        if (gx < s.X && gy < s.Y) {
            OT* row = out + ((size_t)c.b * V + ((size_t)gz * s.X + (c.x0 + lx)) * s.Y + c.y0);
            OT* o = row + (unsigned)(h * s.Y + 4 * n + 2 * (q & 1));
            float t0 = 0.0f, t1 = 0.0f;
            asm volatile("" : "+v"(t0), "+v"(t1));
            if (s.head & 1) { t0 += (float)load_now(o); t1 += (float)load_now(o + 1); }
            if (s.head & 2) { t0 = relu_tanh(t0); t1 = relu_tanh(t1); }
            if constexpr (sizeof(OT) == 4) *reinterpret_cast<float2*>(o) = make_float2(t0, t1);
            else *reinterpret_cast<double2*>(o) = make_double2((double)t0, (double)t1);
        }
    }
}

// The row bits of a window of kRows + 8 halo rows that starts at row r = 4 a + c, in the row masks' layout (byte xr, bit q =
// row 4 xr + q): a constant selected by c, moved up a bytes (rows past 15 fall off the top, as they do not exist).  Scalar;
// the callers pass c in a form that shows which values it can take (rebuilt with shifts and ors per round it was ~10 scalar
// instructions).
constexpr uint32_t zrow_bits(uint32_t w) {
    return (w & 0xfu) | ((w & 0xf0u) << 4) | ((w & 0xf00u) << 8) | ((w & 0xf000u) << 12);
}
template <int kRows>
__device__ __forceinline__ uint32_t zwindow_mask(int c, int a) {
    constexpr uint32_t W = (1u << (8 + kRows)) - 1u;
    static_assert(kRows == 1 || kRows == 2, "a window of 9 or 10 rows: W << 3 stays inside 16 bits");
    const uint32_t m = c == 0 ? zrow_bits(W) : c == 1 ? zrow_bits(W << 1) : c == 2 ? zrow_bits(W << 2) : zrow_bits(W << 3);
    return m << (8 * a);
}

// LDS counter add by ONE lane, as the instruction it is: hipcc's atomic optimiser turns `if (lane == 0) atomic_add` into a
// cross-lane aggregation (mbcnt, bcnt, a second exec dance: ~12 instructions per signal, four signals per ticket)
// kTag names the hand-over in the ISA (a comment inside the asm block: `; @zw:add<kTag>`), for tools/zwalk_handover_audit.py:
//   1 landed[pass][slot] (LDS-DMA -> fold)   2 folded[slot] (fold -> rounds, and -> the LDS-DMA that reuses the raw slot)
//   3 read[slot] (rounds -> the fold that overwrites their planes)
template <int kTag>
__device__ __forceinline__ void lds_add_lane0(int* counter, int value, int lane) {
    if (lane == 0) {
        const uint32_t a = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) int*)counter;
        asm volatile("; @zw:add%c2\n\tds_add_u32 %0, %1" ::"v"(a), "v"(value), "i"(kTag) : "memory");
    }
}

// kH: x-rows per round (2: eight accumulator tiles, as the tile kernels; 1: four -- half the registers, more waves per SIMD);
// kR: rounds a ticket runs back to back (x-rows kH kR tk .. + kH kR - 1: the ticket's claim, dependency check, pass and
// ring addresses are paid once for all of them -- [measured] one round of one x-row per ticket spent more vector
// instructions on that bookkeeping (120) than on its 48 MFMAs' operands (74));  kW: waves per workgroup.
// A slot has 8 / (kH kR) tickets; its four LDS-DMA / fold passes are dealt over them.
// kAct: the launch writes the per-kernel activations (false: `act` is null -- the head-only form of the headline path.  A
// compile-time fact because the activations' four 64-bit row addresses per lane are loop invariants the compiler computes
// per ticket whether or not a round stores through them: [measured in the ISA] 35 of the 75 vector instructions of a
// ticket's round set-up, and two spilled register pairs).
template <typename OT, int kH, int kR, int kW, bool kAct>
__global__ __launch_bounds__(64 * kW) void conv_occ_i8z_kernel(const uint8_t* __restrict__ x,
                                                                const float* __restrict__ lambdas,
                                                                const uint8_t* __restrict__ prep, ZShape zs,
                                                                OT* __restrict__ act_arg, OT* __restrict__ out) {
    if (!zs.gate.pass()) return;
    OT* const act = kAct ? act_arg : nullptr;
    // kLean (round 7): the head-only form takes the ticket's verdict first and stores an all-empty ticket's rows from one row
    // address (THE TICKET'S VERDICT FIRST, below).  The activations form keeps the round-6 ticket as it was: with the lean
    // ticket's code in, the (1, 2, 12) activations instantiation stored a stray + 0.0 into single activations of kernel 13 on
    // some launches ([measured] tests/test_gpu_conv_zwalk_skip.py::test_half_occupancy_skips_nothing, also with
    // conv_i8z_dense = 1, i.e. with none of the new code executed: a sensitivity of the generated code that is not understood),
    // so nothing about that form's code is changed.
    constexpr bool kLean = !kAct;
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    constexpr int kNT = 64 * kW;              // threads
    constexpr int kTPS = kZTX / (kH * kR);    // tickets per slot: 8 or 4
    constexpr int kTShift = kTPS == 8 ? 3 : 2;
    // (A ticket that carries passes carries ONE LDS-DMA pass and ONE fold pass.  The two-passes shape -- four rounds per
    // ticket, two tickets per slot -- is gone: slowest of all (109-123 us), and with two tickets per slot the end of a stream
    // can reach the read[] hazard described at the dependency check; DESIGN section 4, tools/debug/zwalk_protocol_sim.py.)
    constexpr int kNVz = 4 * kH;              // accumulator tiles per round
    static_assert(kH == 1 || kH == 2, "rounds of one or two x-rows");
    static_assert(kTPS * kH * kR == kZTX && (kTPS == 8 || kTPS == 4), "ticket shape");
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // LDS carve-up
    uint4* Wd = reinterpret_cast<uint4*>(lds);                                   // [4][3][64] x 16 B
    int4* jobtab = reinterpret_cast<int4*>(Wd + kFoldSteps * 3 * 64);            // [kZMaxJobs] (b, x0, y0, zs); THE BALANCED DEAL's
                                                                                 // table (one y tile: y0 = 0) holds a | len << 8 of
                                                                                 // TRIMMED JOBS in the y0 field
    float* scale = reinterpret_cast<float*>(jobtab + kZMaxJobs);                 // [16]
    float* lamsc = scale + 16;                                                   // [16]
    float* lamhi = lamsc + 16;                                                   // [16] (+ 64 bytes spare)
    double* bnd = reinterpret_cast<double*>(lamhi + 32);                         // [16]
    int* cnt = reinterpret_cast<int*>(bnd + 16);                                 // [128] counters, see below
    int4* chk = reinterpret_cast<int4*>(cnt + 128);                              // [64] the dependency check's lane roles
    int4* ltab = chk + 64;                                                       // [64] a lane's constants (n 16, q 256, 4 n + q, -)
    int4* stab = ltab + 64;                                                      // [16][4] ring offsets of (sigma & 15, lane group q)
    uint32_t* rowmask = reinterpret_cast<uint32_t*>(stab + 64);                  // [16] non-empty rows of the plane in ring slot u & 15:
                                                                                 // byte xr, bit q = row 4 xr + q (+ 64 B spare: the
                                                                                 // rings stay 128-byte aligned)
    uint8_t* raw = reinterpret_cast<uint8_t*>(rowmask + 32);                     // [16][16 rows][96 B]
    uint8_t* Yc = raw + kZRing * kZRawPlane;                                     // [16][16 rows][16 lanes] x 4 B (+ 32 B per plane)
    uint8_t* Yq = Yc + kZRing * kZYcPlane;                                       // [16][16 rows][16 lanes] x 16 B
    // counters: [0..15] folded[slot]: fold passes of the planes that lived there (4 per plane);
    //           [16..31] read[slot]: tickets of the slots s = slot (mod 16) that are through with their ring reads (kTPS per slot);
    //           [32..95] landed[pass][slot]: LDS-DMA passes arrived;  [96] ticket counter;  [97] asymmetric bank;  [98] a spin gave up
    //           [99] can_skip;  [100] rounds run, [101] rounds skipped, [102] waves that have added theirs;  [103] live jobs (DEAD JOBS;
    //           THE BALANCED DEAL: the live jobs of this workgroup's share);  [104] THE BALANCED DEAL: jobs in this workgroup's table.
    //           [105] TRIMMED JOBS: planes of the workgroup's stream (the sum of len + 8 over its live jobs);  [106], [107] planes
    //           streamed / trimmed away, for the device's count.
    //           [103] / [104] are written by wave 0 ahead of the prologue's second barrier and, when the launch may not skip, once
    //           more by wave 0 behind the verdict (the static table and its count).  `dealt` -- which poison_jobs walks -- is read
    //           from [104] right behind the second barrier and again behind the __syncthreads that ends the prologue.  A slow
    //           wave's first read may already see the static count: wave 0 writes it only once it is past the verdict, i.e. in a
    //           launch that does not decline (the verdict is workgroup-uniform), so no wave poisons with it, no wave requests
    //           planes early (each finds the same coefficients not finite), and every wave reads it again before it is used.
    int* const ticket_ctr = cnt + 96;

#ifdef SN_CONV_TIMING
    if (lane < 8 && wave < 8) g_i8s_w[(blockIdx.x * 8 + wave) * 8 + lane] = 0;
#define SN_ZT(k, t0) do { if (lane == 0 && wave < 8) g_i8s_w[(blockIdx.x * 8 + wave) * 8 + (k)] += clock64() - (t0); } while (0)
#define SN_ZNOW() clock64()
#else
#define SN_ZT(k, t0) do { (void)(t0); } while (0)
#define SN_ZNOW() 0ull
#endif
    SN_ST(0);
    const size_t V = (size_t)zs.Z * zs.X * zs.Y;
    const int grid = (int)gridDim.x;
    int dealt = (int)blockIdx.x < zs.njobs ? (zs.njobs - 1 - (int)blockIdx.x) / grid + 1 : 0;   // jobs of this workgroup
    const int dealt_static = dealt;           // (THE BALANCED DEAL changes `dealt`)
    int my_jobs = dealt;                      // ... and those it walks (DEAD JOBS below: the live ones)
    int NPL = my_jobs * zs.PL;                // planes of this workgroup's stream
    int nslots = NPL + kZD;                   // slots (the last kZD only flush rounds)
    // DEAD JOBS (round 8, head-only form, zs.fill_dead: the dealt plan).  A job is DEAD when no byte of x[b] is set in planes
    // zs - 4 .. zs + LZ + 3, rows x0 - 4 .. x0 + 11, y0 - 4 .. y0 + 67 (clipped to the grid): the union of the windows of all its
    // rounds under the conservative row rule above, so every one of its rounds would be skipped.  The workgroup checks its own
    // jobs in its prologue (16-byte loads of the rows' pieces -- the LDS-DMA's pieces -- ahead of the blob copy), moves
    // the live ones to the front of its job table, requests the first planes of the first LIVE job only then, and fills a dead
    // job's outputs with what its rounds would have stored (the lean ticket's constant, or zero_round's load-add-activate under
    // head & 1) with 16-byte stores.  A launch that declines, or may not skip (can_skip), treats every job as live.  Nothing of
    // the ticket loop knows: it walks a shorter stream.  A workgroup whose FIRST job is live -- it stays the first whatever the
    // launch decides -- requests that job's planes as soon as the flags are known, so its LDS-DMA flies through the verdict as
    // the parent's does.  The job flags live in the folded ring, which nothing uses before the first fold pass.
    const bool fill_dead = kLean && zs.fill_dead != 0;
    int* const live = reinterpret_cast<int*>(Yq);   // [kZMaxJobs], fill_dead only
    if (tid < 128) cnt[tid] = 0;
    if (tid >= 128 && tid < 192) {
        // lane roles of a ticket's dependency check (one LDS read of counter `idx`, expected value `expect`):
        //   lanes 0..8    folded[plane sigma + i]  for a round (its nine planes)
        //   lanes 16..24  read[slot s - 14 + i]    for a fold (the readers of the plane it overwrites)
        //   lane 32       landed[pass][plane s]    for a fold (its raw rows)
        //   lane 40       folded[plane sd - 16]    for an LDS-DMA (the raw slot it overwrites has been folded)
        //   lane 48       read[slot s - 16]        for EVERY ticket (need bit 8): the previous owner of read[s & 15] is complete
        //                 before this ticket may add to it.  read[] is shared by the slots v and v + 16; a ticket with nothing
        //                 to do (the 8 trailing planes of a job, the flush slots) used to report at once, and at the END of a
        //                 stream such reports could complete read[v & 15] while a round of slot v was still reading: the folds of
        //                 planes v + 5 .. were then let loose one report early (round 4, found by the hazard model,
        //                 tools/debug/zwalk_protocol_sim.py --hole: reachable with two tickets per slot or 16 waves, not with
        //                 the shipped 12 waves x 4 or 8 tickets -- there every other wave is held by a fold that waits for v).
        //                 Costs nothing: one more lane of the same LDS read.
        // as (offset of the stream position from s, counter base, need bit | mask of 16 xr0, shift of the expected count):
        // read back per ticket instead of being rebuilt from the lane id ([measured in the ISA] 42 vector instructions)
        const int l = tid - 128, i = l & 15, role = l >> 4;
        int4 e = make_int4(0, 0, 0, 0);
        if (role == 0 && i <= 8) e = make_int4(i - kZD, 0, 1, 2);
        if (role == 1 && i <= 8) e = make_int4(i - kZRing + kZLag, 16, 2, kTShift);   // (readers of plane s - 16: slots s - 16 + kZLag ..)
        if (l == 32) e = make_int4(0, 32, 2 | 0x30, 0);
        if (l == 40) e = make_int4(kZDD - 16, 0, 4, 2);
        if (l == 48) e = make_int4(-kZRing, 16, 8, kTShift);
        chk[l] = e;
    }
    // What a round's ring addresses are built from, read back per ticket (two ds_read_b128) instead of being rebuilt from the
    // lane id: kept live through a ticket's rounds such values were spilled, recomputed they were [measured in the ISA, round
    // 4] 39 vector instructions of a ticket whose launch is bound by instruction issue (DESIGN section 4).
    //   ltab[lane]            = (n 16, q 256, 4 n + q, -)
    //   stab[sigma & 15][q]   = byte offsets of the lane group's two planes dz = 2 q, 2 q + 1 in the folded rings:
    //                           (sA YqPlane, sA YcPlane, sB YqPlane, sB YcPlane), sA = (sigma + 2 q) & 15, sB = (sA + 1) & 15
    if (tid >= 192 && tid < 256) {
        const int l = tid - 192;
        ltab[l] = make_int4((l & 15) * 16, (l >> 4) * 256, 4 * (l & 15) + (l >> 4), (l >> 4) * 16);
    }
    if (tid >= 256 && tid < 320) {   // (LDS byte addresses: the rings' bases are folded in)
        const int e = tid - 256, sg = e >> 2, qq = e & 3;
        const int a = (sg + 2 * qq) & 15, b = (sg + 2 * qq + 1) & 15;
        const int yq0 = (int)(uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint8_t*)Yq;
        const int yc0 = (int)(uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint8_t*)Yc;
        stab[e] = make_int4(yq0 + a * kZYqPlane, yc0 + a * kZYcPlane, yq0 + b * kZYqPlane, yc0 + b * kZYcPlane);
    }
    // job k of this workgroup under the static plan: (b, x0, y0, zs)
    auto static_job = [&](int k) -> int4 {
        int j = zjob_id(zs, (int)blockIdx.x, k, grid);
        int xt, yt, sg;
        if (zs.deal) {
            const int ncol = zs.B * zs.nxt * zs.nyt;
            sg = j / ncol; j -= sg * ncol;
            xt = j % zs.nxt; j /= zs.nxt;
            yt = j % zs.nyt; j /= zs.nyt;
            xt = (xt + zs.deal_shift * sg) % zs.nxt;
        } else {
            xt = j % zs.nxt; j /= zs.nxt;
            yt = j % zs.nyt; j /= zs.nyt;
            sg = j % zs.nseg; j /= zs.nseg;
        }
        return make_int4(j, xt * kZTX, yt * TY, sg * zs.LZ);
    };
    if (tid < my_jobs) jobtab[tid] = static_job(tid);
    // THE BALANCED DEAL (round 9, zs.bal): the job table comes from the tile's row bits, see below; no byte check
    const bool bal = kLean && fill_dead && zs.bal != 0;
    if constexpr (kLean) {
        if (fill_dead && !bal)
            for (int i = tid; i < kZMaxJobs; i += kNT) live[i] = 0;
    }
    lds_barrier();

    // the job a plane / an output belongs to: (b, x0, y0, zs) in scalar registers, re-read from the table only when the
    // job index changes (a table read per ticket was an exposed LDS round trip)
    struct JobRegs { int k, b, x0, y0, zs; };
    auto job_fetch = [&](JobRegs& jr, int k) -> bool {   // (true: the job changed)
        if (k == jr.k) return false;
        const int4 jb = jobtab[k];
        jr.b = __builtin_amdgcn_readfirstlane(jb.x); jr.x0 = __builtin_amdgcn_readfirstlane(jb.y);
        jr.y0 = __builtin_amdgcn_readfirstlane(jb.z); jr.zs = __builtin_amdgcn_readfirstlane(jb.w);
        jr.k = k;
        return true;
    };
    JobRegs jd{-1, 0, 0, 0, 0}, jr{-1, 0, 0, 0, 0};
    // kLean, THE CURSOR (TRIMMED JOBS): a job's stream positions [s0, end) and its outputs `len` ride beside its registers, and
    // `zs` is the grid plane of its output 0 (a trimmed job: a, else the segment's first plane).  A wave's stream positions only
    // grow -- the prologue's planes in order, then sd = s + kZDD of ever later tickets; sigma likewise -- so it steps to the next
    // job while the position is at or past `end`: one LDS read when the job changes, none otherwise.  Every position asked for
    // lies below NPL, i.e. inside a live job of the table.
    bool bal_keep = false;   // THE BALANCED DEAL's table stands (the launch may skip): its y0 fields hold a | len << 8
    struct JobSpan { int next, s0, end, len; };
    JobSpan sd_{0, 0, 0, 0}, sr_{0, 0, 0, 0};
    auto job_step = [&](JobRegs& j, JobSpan& sp) {
        const int4 jb = jobtab[sp.next & (kZMaxJobs - 1)];   // (the mask: a table address with an immediate offset)
        int a = jb.w, len = zs.LZ, y0 = jb.z;
        if (bal_keep) {
            a = jb.z & 255;
            len = jb.z >> 8;
            y0 = 0;
        }
        j.b = __builtin_amdgcn_readfirstlane(jb.x); j.x0 = __builtin_amdgcn_readfirstlane(jb.y);
        j.y0 = __builtin_amdgcn_readfirstlane(y0); j.zs = __builtin_amdgcn_readfirstlane(a);
        j.k = sp.next++;
        sp.len = __builtin_amdgcn_readfirstlane(len);
        sp.s0 = sp.end;
        sp.end = sp.s0 + sp.len + 8;
    };
    // kLean: the jobs' tile bases x + b V and out + b V are 64-bit scalars formed when the job changes, not per pass and per
    // round (round 7: the product b V was formed three times per ticket); everything below adds 32-bit offsets (the host
    // checks Z X Y < 2^31)
    const uint8_t* xb = x;
    OT* ob = nullptr;

    // ---- LDS-DMA of four raw rows (pass xr) of plane u: 24 lanes x 16 B, rows contiguous in the ring slot
    auto dma_pass = [&](int u, int xr, int ln) {
        const int dl_row = (ln * 43) >> 8, dl_i = ln - dl_row * kRowPieces;   // ln / 6, ln % 6 for ln < 24 (the lanes that take part)
        int p;
        if constexpr (kLean) {
            while (u >= sd_.end && sd_.next < dealt) {   // (the bound cannot bind: u < NPL; it keeps a wrong table from spinning)
                job_step(jd, sd_);
                xb = x + (size_t)jd.b * V;
            }
            p = u - sd_.s0;
        } else {
            const int k = (int)__umulhi((unsigned)u, zs.pl_magic);
            p = u - k * zs.PL;
            job_fetch(jd, k);
        }
        const int gz = jd.zs - 4 + p;
        const int gx = jd.x0 - 4 + 4 * xr + dl_row, gy = jd.y0 - PYA + 16 * dl_i;
        const bool ok = (unsigned)gz < (unsigned)zs.Z && (unsigned)gx < (unsigned)zs.X && (unsigned)gy < (unsigned)zs.Y;
        uint8_t* const dst = raw + (u & 15) * kZRawPlane + xr * (4 * DW * 4);   // wave-uniform; lane l's piece at + 16 l
        const uint32_t lds_uni = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint8_t*)dst);
        // tile base (scalar, 64-bit) + a 32-bit offset inside the tile (the host checks Z X Y < 2^31); pieces outside the grid
        // are fetched from the 16 zero bytes of the caller's blob (a kernel argument: no GOT load for a zero block)
        const uint8_t* const tile = kLean ? xb : x + (size_t)jd.b * V;
        const uint8_t* src = ok ? tile + (unsigned)((gz * zs.X + gx) * zs.Y + gy) : prep + kPrepZero;
        if (ln < 4 * kRowPieces) {
            uint32_t m0_saved;
            asm volatile("; @zw:dma\n\ts_mov_b32 %0, m0\n\ts_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %2, off\n\t"
                         "s_mov_b32 m0, %0"
                         : "=&s"(m0_saved) : "s"(lds_uni), "v"(src) : "memory");
        }
    };
    // ---- fold pass xr of plane u: lane (q, n) folds row 4 xr + q
    auto fold_pass = [&](int u, int xr, int ln) {
        const int n = ln & 15, q = ln >> 4;
        const uint32_t* p = reinterpret_cast<const uint32_t*>(raw + (u & 15) * kZRawPlane + (4 * xr + q) * (DW * 4) + (n + D0) * 4);
        const uint32_t R0 = p[0], R1 = p[1], R2 = p[2];
        // which of the pass's four rows hold a set voxel: lane group q is row 4 xr + q (scalar arithmetic on the ballot)
        const unsigned long long any = __builtin_amdgcn_ballot_w64((R0 | R1 | R2) != 0u);
        // (s_quadmask: bit i = OR of the source's bits 4 i .. 4 i + 3; twice: bit q = OR of the 16 lanes of group q)
        unsigned long long any4;
        uint32_t rowbits;
        asm("s_quadmask_b64 %0, %1" : "=s"(any4) : "s"(any) : "scc");
        asm("s_quadmask_b32 %0, %1" : "=s"(rowbits) : "s"((uint32_t)any4) : "scc");
        uint4 f;
        f.x = R0 + __builtin_amdgcn_perm(R2, R1, 0x01020304u);
        f.y = __builtin_amdgcn_alignbyte(R1, R0, 1) + __builtin_amdgcn_perm(R2, R1, 0x02030405u);
        f.z = __builtin_amdgcn_alignbyte(R1, R0, 2) + __builtin_amdgcn_perm(R2, R1, 0x03040506u);
        f.w = __builtin_amdgcn_alignbyte(R1, R0, 3) + __builtin_amdgcn_perm(R2, R1, 0x04050607u);
        *reinterpret_cast<uint4*>(Yq + (u & 15) * kZYqPlane + (4 * xr + q) * kZYqRow + n * 16) = f;
        *reinterpret_cast<uint32_t*>(Yc + (u & 15) * kZYcPlane + (4 * xr + q) * kZYcRow + n * 4) = R1;
        if (lane == 0) reinterpret_cast<uint8_t*>(rowmask)[(u & 15) * 4 + xr] = (uint8_t)rowbits;   // (ahead of the folded[] report)
    };

    // ---- NaN over everything this workgroup owns in `out` / `act` (cold: a spin gave up, or a `served` launch declined)
    auto poison_jobs = [&]() {
        const OT nan = (OT)__int_as_float(0x7fc00000);
        for (int k = 0; k < dealt; ++k) {   // (every job the workgroup was dealt: walked or filled)
            int4 jb = jobtab[k];
            if (bal) jb.z = 0;   // (THE BALANCED DEAL: one y tile, and its table's y0 fields hold TRIMMED JOBS' ranges)
            for (int r = wave; r < zs.LZ * kZTX; r += kW) {
                const int gz = jb.w + (r >> 3), gx = jb.y + (r & 7), gy = jb.z + lane;
                if (gz >= zs.Z || gx >= zs.X || gy >= zs.Y) continue;
                const size_t off = ((size_t)gz * zs.X + gx) * zs.Y + gy;
                if (out) out[(size_t)jb.x * V + off] = nan;
                if (act)
                    for (int g = 0; g < zs.G; ++g) act[((size_t)jb.x * zs.Gtot + zs.g0 + g) * V + off] = nan;
            }
        }
    };

    // ---- prologue: the first planes' raw rows are requested before anything else; the blob is copied while they fly
    // (fill_dead: the planes are requested once the first live job is known, below; here the check's loads go out instead)
    int npre = NPL < kZPre ? NPL : kZPre;
    if (!fill_dead)
        for (int p = wave; p < 4 * npre; p += kW) dma_pass(p >> 2, p & 3, lane);
    // DEAD JOBS, the check: OR of the bytes of the operand regions of jobs k0 and k0 + 1 that this thread reads.  A thread keeps
    // one (row, piece) of the region -- kNT is a multiple of 128 = 16 rows x 8 piece slots, 6 of them pieces -- and takes every
    // (kNT / 128)-th plane; the pieces are the LDS-DMA's (16 bytes from y0 - 16 on, wholly inside or outside the grid), of which
    // the first and the last count with 4 bytes (y0 - 4 .., .. y0 + 67).  Whatever lies outside the grid or the region is read
    // again from the start of the tile and dropped: every load is unconditional, a batch of 2 x 8 is in flight at once.
    auto region_or2 = [&](int k0, uint32_t& a0, uint32_t& a1) {
        static_assert(kNT % 128 == 0, "a thread's (row, piece) is the same for every plane it takes");
        constexpr int kStep = kNT / 128, kBatch = 8;
        const int pc = tid & 7, row = (tid >> 3) & 15;
        const bool two = k0 + 1 < dealt;
        const int4 j0 = jobtab[k0], j1 = jobtab[two ? k0 + 1 : k0];
        // (the thread's row and piece inside the grid?  its byte offset in plane 0 of the tile, and which dwords count)
        const int gx0 = j0.y - 4 + row, gy0 = j0.z - PYA + 16 * pc, gx1 = j1.y - 4 + row, gy1 = j1.z - PYA + 16 * pc;
        const bool in0 = pc < kRowPieces && (unsigned)gx0 < (unsigned)zs.X && (unsigned)gy0 < (unsigned)zs.Y;
        const bool in1 = two && pc < kRowPieces && (unsigned)gx1 < (unsigned)zs.X && (unsigned)gy1 < (unsigned)zs.Y;
        const int plane = zs.X * zs.Y;
        const uint8_t* const t0 = x + (size_t)j0.x * V + (unsigned)(in0 ? gx0 * zs.Y + gy0 : 0);
        const uint8_t* const t1 = x + (size_t)j1.x * V + (unsigned)(in1 ? gx1 * zs.Y + gy1 : 0);
        const uint32_t kx = pc == kRowPieces - 1 ? ~0u : pc == 0 ? 0u : ~0u, kyz = (pc == 0 || pc == kRowPieces - 1) ? 0u : ~0u,
                       kw = pc == 0 ? ~0u : pc == kRowPieces - 1 ? 0u : ~0u;
#pragma unroll 1
        for (int pl0 = tid >> 7; pl0 < zs.PL; pl0 += kStep * kBatch) {
            // a plane outside the region or the grid: the thread reads plane 0 of its tile again and drops what it gets
            uint4 v0[kBatch], v1[kBatch];
            bool ok0[kBatch], ok1[kBatch];
#pragma unroll
            for (int u = 0; u < kBatch; ++u) {
                const int pl = pl0 + u * kStep, gz0 = j0.w - 4 + pl, gz1 = j1.w - 4 + pl;
                ok0[u] = in0 && pl < zs.PL && (unsigned)gz0 < (unsigned)zs.Z;
                ok1[u] = in1 && pl < zs.PL && (unsigned)gz1 < (unsigned)zs.Z;
                v0[u] = *reinterpret_cast<const uint4*>(t0 + (unsigned)(ok0[u] ? gz0 * plane : 0));
                v1[u] = *reinterpret_cast<const uint4*>(t1 + (unsigned)(ok1[u] ? gz1 * plane : 0));
            }
#pragma unroll
            for (int u = 0; u < kBatch; ++u) {
                const uint32_t w0 = (v0[u].x & kx) | ((v0[u].y | v0[u].z) & kyz) | (v0[u].w & kw);
                const uint32_t w1 = (v1[u].x & kx) | ((v1[u].y | v1[u].z) & kyz) | (v1[u].w & kw);
                a0 |= ok0[u] ? w0 : 0u;
                a1 |= ok1[u] ? w1 : 0u;
            }
        }
    };
    // (one ballot per wave, then one lane sets the job's flag: every writer stores the same 1, an OR without the atomic)
    auto region_report = [&](int k, uint32_t a) {
        if (__builtin_amdgcn_ballot_w64(a != 0u) != 0ull && lane == 0) live[k] = 1;
    };
    // THE BALANCED DEAL (round 9, head-only form; host guard in conv_i8s.hip: one y tile, Z <= 64, X <= 64, as many columns
    // as workgroups, at most kZBalJobs jobs per tile).  The nxt workgroups that the static deal gives one tile's columns share
    // that tile's nxt x nseg jobs by cost instead.  Every one of them forms the SAME plan from the same 512 bytes -- the tile's
    // row bits, rows[b][z][w]: bit x % 32 of word x / 32 set iff plane z, row x holds a set voxel (a superset is allowed: it costs
    // time, never a result) -- in its wave 0, and keeps its share; nothing is exchanged.  Lane z holds plane z's 64 row bits and
    // their nine-plane window W (the OR over z - 4 .. z + 4); lane jj holds job jj = sg nxt + xs, the static deal's job number
    // sg ncol + b nxt + xs: column xt = (xs + shift sg) % nxt, planes sg LZ ...  Per column, ballots over the planes give
    //   live        a row bit in planes zs - 4 .. zs + LZ + 3, rows x0 - 4 .. x0 + 11: DEAD JOBS' rule (one y tile: every y counts)
    //   rounds_run  the rounds (x-rows h .. h + kH - 1, plane z) with a bit of W[z] in rows h .. h + kH + 7: EMPTY WINDOWS' rule
    // and  cost = live ? kBalPlane PL + kBalRound rounds_run : kBalFill  (integers: tools/debug/zwalk_balanced_model.py deals
    // the same).  Jobs in the order (cost descending, job number ascending) go one by one to the workgroup with the smallest
    // load, ties to the lowest.  A workgroup's table holds its jobs in that order: the live ones come first by themselves (a
    // live job costs more than any dead one).  The table is written over the static one, which wave 0 restores if the launch may
    // not skip (then every job is live and the static deal runs, as without bits).
    if constexpr (kLean) {
        if (bal && wave == 0) {
            const int nxt = zs.nxt, nj = nxt * zs.nseg;
            const int c0 = zjob_id(zs, (int)blockIdx.x, 0, grid);   // (ncol == grid: the workgroup's column number)
            const int b = c0 / nxt, me = c0 - b * nxt;
            const int wx = (zs.X + 31) >> 5;
            unsigned long long r = 0ull;
            if (lane < zs.Z) {
                const uint32_t* p = zs.rows + ((size_t)b * zs.Z + lane) * wx;
                r = p[0];
                if (wx > 1) r |= (unsigned long long)p[1] << 32;
            }
            auto up = [&](unsigned long long v, int d) { const unsigned long long t = __shfl_up(v, d, 64); return lane >= d ? t : 0ull; };
            auto down = [&](unsigned long long v, int d) { const unsigned long long t = __shfl_down(v, d, 64); return lane + d < 64 ? t : 0ull; };
            const unsigned long long w3 = r | up(r, 1) | down(r, 1);
            // (w3 of lane z covers planes z - 1 .. z + 1; the lanes three away, CLAMPED to the wave: near an end of the wave the
            // end lane's two planes are inside the window, and w3 of a lane that does not exist would have held one of them)
            const unsigned long long W = w3 | __shfl(w3, lane >= 3 ? lane - 3 : 0, 64) | __shfl(w3, lane + 3 < 64 ? lane + 3 : 63, 64);
            // this lane's job
            const int sg = lane / nxt, xs = lane - sg * nxt, xt_mine = (xs + zs.deal_shift * sg) % nxt, z0 = sg * zs.LZ;
            auto zbits = [](int lo, int hi) -> unsigned long long {   // planes lo .. hi - 1, 0 <= lo, hi <= 64
                if (hi <= lo) return 0ull;
                return (hi >= 64 ? ~0ull : (1ull << hi) - 1ull) & ~((1ull << lo) - 1ull);
            };
            const int z1 = z0 + zs.LZ < zs.Z ? z0 + zs.LZ : zs.Z;
            const unsigned long long zrun = zbits(z0 < 64 ? z0 : 64, z1),
                                     zreg = zbits(z0 - 4 > 0 ? (z0 - 4 < 64 ? z0 - 4 : 64) : 0, z1 + 4 < zs.Z ? z1 + 4 : zs.Z);
            bool lv = false;
            int rounds = 0;
            unsigned long long lvw = 0ull;   // TRIMMED JOBS: this job's live output planes
#pragma unroll 1
            for (int xt = 0; xt < nxt; ++xt) {
                const int x0 = xt * kZTX;
                // halo rows x0 - 4 .. x0 + 11 of this lane's plane: bit i = row x0 - 4 + i (rows outside the grid hold no bit)
                const uint32_t raw16 = (uint32_t)(x0 >= 4 ? r >> (x0 - 4) : r << 4) & 0xffffu;
                const uint32_t win16 = (uint32_t)(x0 >= 4 ? W >> (x0 - 4) : W << 4) & 0xffffu;
                const bool is_mine = xt == xt_mine;
                const unsigned long long lb = __builtin_amdgcn_ballot_w64(raw16 != 0u);
                if (is_mine) lv = (lb & zreg) != 0ull;
                // (the OR over h of the rounds' ballots below: a plane with no bit here has every round empty, for either kH)
                const unsigned long long wl = __builtin_amdgcn_ballot_w64(win16 != 0u);
                if (is_mine) lvw = wl & zrun;
                const int nrows = zs.X - x0 < kZTX ? zs.X - x0 : kZTX;
#pragma unroll
                for (int h = 0; h < kZTX; h += kH) {
                    if (h < nrows) {
                        const unsigned long long rb = __builtin_amdgcn_ballot_w64((win16 & (((1u << (kH + 8)) - 1u) << h)) != 0u);
                        if (is_mine) rounds += __builtin_popcountll(rb & zrun);
                    }
                }
            }
            const uint32_t cost = lv ? (uint32_t)(kBalPlane * zs.PL + kBalRound * rounds) : (uint32_t)kBalFill;
            // rank in (cost descending, job number ascending): keys are distinct, a lane without a job has none
            const uint32_t key = lane < nj ? cost * 64u + (uint32_t)(63 - lane) : 0u;
            int rank = 0;
#pragma unroll 1
            for (int i = 0; i < nj; ++i) rank += (uint32_t)__builtin_amdgcn_readlane((int)key, i) > key ? 1 : 0;
            // lane s: the job of rank s
            uint32_t sk = 0u;
            if (lane < nj) sk = (uint32_t)__builtin_amdgcn_ds_permute(rank * 4, (int)key);
            // the deal: lanes 0 .. nxt - 1 hold the workgroups' loads; the smallest (load, workgroup) of the first eight lanes by
            // three DPP steps (lane ^ 1, lane ^ 2, the other quad of the half row)
            uint32_t load = lane < nxt ? 0u : 0x0fffffffu;
            int owner = -1;
#pragma unroll 1
            for (int s = 0; s < nj; ++s) {
                const uint32_t cs = (uint32_t)__builtin_amdgcn_readlane((int)sk, s) >> 6;
                uint32_t m = (load << 3) | (uint32_t)(lane & 7);
                uint32_t o = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)m, 0xB1, 0xf, 0xf, false);
                m = o < m ? o : m;
                o = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)m, 0x4E, 0xf, 0xf, false);
                m = o < m ? o : m;
                o = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)m, 0x141, 0xf, 0xf, false);
                m = o < m ? o : m;
                const int arg = __builtin_amdgcn_readfirstlane((int)m) & 7;
                if (lane == arg) load += cs;
                if (lane == s) owner = arg;
            }
            const bool mine = lane < nj && owner == me;
            const unsigned long long mb = __builtin_amdgcn_ballot_w64(mine);
            const unsigned long long lvb = __builtin_amdgcn_ballot_w64(mine && (sk >> 6) > (uint32_t)kBalFill);
            const int pos = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(mb >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mb, 0u));
            const int n_mine = __builtin_popcountll(mb);
            // TRIMMED JOBS: this lane's job streams outputs [ta, ta + tlen) -- from its first to its last live plane, at least
            // min(8, LZ) of them, moved down where the segment ends first; the whole segment without the option (or should the
            // two verdicts ever disagree: lv is the one the deal and the fill go by).  Lane s fetches its job's pair from lane jj.
            int ta = z0, tlen = zs.LZ;
            if (zs.trim && lvw != 0ull) {
                const int lmin = zs.LZ < 8 ? zs.LZ : 8;
                ta = __builtin_ctzll(lvw);
                tlen = 64 - __builtin_clzll(lvw) - ta;
                tlen = tlen < lmin ? lmin : tlen;
                if (ta + tlen > z1) ta = z1 - tlen;
            }
            const int tr = __shfl(ta | (tlen << 8), lane < nj ? 63 - (int)(sk & 63u) : 0, 64);
            const bool mine_live = mine && (sk >> 6) > (uint32_t)kBalFill;
            if (mine_live) atomicAdd(&cnt[105], (tr >> 8) + 8);   // (few lanes, once per launch)
            if (mine) {
                const int jj = 63 - (int)(sk & 63u);
                const int jsg = jj / nxt, jxs = jj - jsg * nxt;
                jobtab[pos] = make_int4(b, ((jxs + zs.deal_shift * jsg) % nxt) * kZTX, tr, jsg * zs.LZ);   // (y0 = 0: tr in its field)
                if (zs.plan_out) zs.plan_out[(size_t)blockIdx.x * (1 + kZBalJobs) + 1 + pos] = jsg * (zs.B * nxt) + b * nxt + jxs;
            }
            if (lane == 0) {
                cnt[103] = __builtin_popcountll(lvb);
                cnt[104] = n_mine;
                if (zs.plan_out) zs.plan_out[(size_t)blockIdx.x * (1 + kZBalJobs)] = n_mine;
            }
        }
    }
    if constexpr (kLean) {
        if (fill_dead && !bal) {
#pragma unroll 1
            for (int k = 0; k < dealt; k += 2) {   // (more than two jobs per workgroup: one more latency per pair)
                uint32_t a0 = 0u, a1 = 0u;
                region_or2(k, a0, a1);
                region_report(k, a0);
                region_report(k + 1, a1);
            }
        }
    }
    {
        const uint4* src = reinterpret_cast<const uint4*>(prep + kPrepWd);
        for (int i = tid; i < kFoldSteps * 3 * 64; i += kNT) Wd[i] = src[i];
        if (tid < 16) {
            scale[tid] = reinterpret_cast<const float*>(prep + kPrepScale)[tid];
            bnd[tid] = reinterpret_cast<const double*>(prep + kPrepBnd)[tid];
            // (the coefficients ride with the blob's loads: read from global by the verdict and again by the head's
            // factors they were two more dependent memory latencies of a prologue that is 5 % of the launch at C2)
            lamhi[16 + tid] = (lambdas && tid < zs.G) ? lambdas[tid] : 0.0f;
            if (tid < zs.G && reinterpret_cast<const int*>(prep + kPrepSym)[tid] == 0) cnt[97] = 1;   // benign race
        }
        // landed[pass][slot] of the prologue's planes.  (zs.dbg & 1, sn_set_option("conv_i8z_inject_fault", 1): plane 0's first
        // pass is never reported -- the test hook that makes a dependency spin give up, so that the loud path can be tested on
        // the product build; costs one compare in the prologue)
        if (tid >= 64 && tid < 128) cnt[32 + tid - 64] = (((tid - 64) & 15) < npre && !((zs.dbg & 1) && tid == 64)) ? 1 : 0;
    }
    lds_barrier();
    bool early = false;   // fill_dead: the first planes are in flight already (job 0 is live and owns all of them)
    // (every coefficient finite, scale not negative: what can_skip asks, below)
    auto coef_finite = [&]() -> bool {
        bool fin = true;
        if (lane < 16) {
            const float sc = scale[lane];
            const float ls = (out && lane < zs.G) ? lamhi[16 + lane] * sc : 0.0f;
            const float lh = 65536.0f * ls;
            auto finite = [](float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; };
            fin = finite(sc) && !(__float_as_uint(sc) >> 31) && finite(ls) && finite(lh);
        }
        return __builtin_amdgcn_ballot_w64(!fin) == 0ull;
    };
    if constexpr (kLean) {
        if (bal) {
            // the balanced table's first job, if live, stays the first whatever the verdict says -- unless the launch may not
            // skip (wave 0 then restores the static table, below): every wave looks at the coefficients itself
            dealt = __builtin_amdgcn_readfirstlane(cnt[104]);
            bal_keep = coef_finite() && !zs.dense;
            // (TRIMMED JOBS: the first live job's own plane count, len_0 + 8, is what must cover the prologue's kZPre planes.
            // len_0 >= min(8, LZ), so with kZPre <= 16 -- asserted here -- len_0 + 8 >= kZPre exactly when PL = LZ + 8 >= kZPre:
            // LZ >= 8 gives len_0 + 8 >= 16; LZ < 8 gives len_0 = LZ.  The uniform test therefore IS the job's own.)
            static_assert(kZPre <= 16, "a trimmed job of min(8, LZ) + 8 planes covers the prologue's planes whenever PL does");
            if (bal_keep && zs.PL >= kZPre && __builtin_amdgcn_readfirstlane(cnt[103]) > 0) {
                early = true;
                for (int p = wave; p < 4 * npre; p += kW) dma_pass(p >> 2, p & 3, lane);
            }
        } else if (fill_dead && dealt > 0 && zs.PL >= kZPre && __builtin_amdgcn_readfirstlane(live[0]) != 0) {
            early = true;   // (npre = kZPre: landed[] above is the stream's, whatever becomes of the other jobs)
            for (int p = wave; p < 4 * npre; p += kW) dma_pass(p >> 2, p & 3, lane);
        }
    }
    {
        // the launch's verdict, for the combined fallback launch enqueued behind this one (conv_i8_fallback_kernel):
        //   0 served here;  1 quantisation bound over the tolerance: the fp32 form;  2 bank not symmetric in x and y: the
        //   unfolded (stride-4) body.  Every workgroup takes the same decision from the same numbers; workgroup 0 writes it.
        // (The stride-4 body used to be inlined here: it wants 243 registers, and under this kernel's budget cost the WALK
        // 80 SGPR spills and ~130 VGPR spills -- [measured] 118.2 -> 110.9 us without it.)
        const bool asym = cnt[97] != 0;
        const bool exceeded = !asym && bound_exceeded<OT>(zs, bnd, lamhi + 16, act, out);
        if (blockIdx.x == 0 && tid == 0) {
            if (zs.route) *zs.route = asym ? 2 : exceeded ? 1 : 0;
            atomicAdd(&g_fold_counts[asym ? 1 : exceeded ? 2 : 0], 1ull);
        }
        if (asym || exceeded) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // do not leave with LDS-DMA in flight
            if (zs.served) {
                // the caller left the fallback launch out on the strength of a verdict that does not hold for THIS bank (a
                // stale cache: e.g. a parameter written through .data): nobody will compute these outputs.  Loud, not quiet.
                poison_jobs();
                if (tid == 0) sn::sticky_latch(zs.sticky, 2, (int)blockIdx.x, asym ? 2 : 1);
            }
            return;
        }
    }
    if (wave == 0) {
        bool fin = true;
        if (tid < 16) {
            const float sc = scale[tid];
            const float ls = (out && tid < zs.G) ? lamhi[16 + tid] * sc : 0.0f;
            const float lh = 65536.0f * ls;
            lamsc[tid] = ls;
            lamhi[tid] = lh;
            auto finite = [](float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; };
            fin = finite(sc) && !(__float_as_uint(sc) >> 31) && finite(ls) && finite(lh);
        }
        // can_skip: an empty round's epilogue is a constant only if coefficient x 0 = + 0 for every coefficient
        const bool all_fin = __builtin_amdgcn_ballot_w64(!fin) == 0ull;
        if (lane == 0) cnt[99] = (all_fin && !zs.dense) ? 1 : 0;
        if constexpr (kLean) {
            if (bal) {
                if (!(all_fin && !zs.dense)) {
                    // THE BALANCED DEAL, declined: every job is live, the static deal runs (NaN / inf propagate as without bits)
                    for (int k = lane; k < dealt_static; k += 64) {
                        jobtab[k] = static_job(k);
                        if (zs.plan_out) zs.plan_out[(size_t)blockIdx.x * (1 + kZBalJobs) + 1 + k] = zjob_id(zs, (int)blockIdx.x, k, grid);
                    }
                    if (lane == 0) {
                        cnt[103] = dealt_static;
                        cnt[104] = dealt_static;
                        if (zs.plan_out) zs.plan_out[(size_t)blockIdx.x * (1 + kZBalJobs)] = dealt_static;
                    }
                }
            } else if (fill_dead) {
                // DEAD JOBS, the job table: live jobs first, in their order, the dead ones behind them, written by this wave from a copy
                // it made (a wave's DS operations execute in order).  A launch that may not skip has no dead job.
                const bool may_skip = all_fin && !zs.dense;
                int4* const old = reinterpret_cast<int4*>(Yq + kZMaxJobs * 4);   // a copy of the table, behind the flags
                int nlive = 0;
#pragma unroll 1
                for (int k0 = 0; k0 < dealt; k0 += 64) {
                    const int k = k0 + lane;
                    const bool lv = k < dealt && (!may_skip || live[k] != 0);
                    if (k < dealt) {
                        old[k] = jobtab[k];
                        live[k] = lv ? 1 : 0;
                    }
                    nlive += __builtin_popcountll(__builtin_amdgcn_ballot_w64(lv));
                }
                int at_live = 0, at_dead = nlive;
#pragma unroll 1
                for (int k0 = 0; k0 < dealt; k0 += 64) {
                    const int k = k0 + lane;
                    const bool in = k < dealt, lv = in && live[k] != 0;
                    const unsigned long long ml = __builtin_amdgcn_ballot_w64(lv), md = __builtin_amdgcn_ballot_w64(in && !lv);
                    const unsigned long long m = lv ? ml : md;
                    const int rank = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
                    if (in) jobtab[(lv ? at_live : at_dead) + rank] = old[k];
                    at_live += __builtin_popcountll(ml);
                    at_dead += __builtin_popcountll(md);
                }
                if (lane == 0) cnt[103] = nlive;
            }
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if constexpr (kLean) {
        if (bal) my_jobs = dealt = __builtin_amdgcn_readfirstlane(cnt[104]);
    }
    if (my_jobs == 0) return;
    const bool can_skip = __builtin_amdgcn_readfirstlane(cnt[99]) != 0;
    int n_run = 0, n_skip = 0;   // this wave's rounds (scalar)
    if constexpr (kLean) {
        if (fill_dead) {
            // DEAD JOBS: the stream is the live jobs'.  Unless they are in flight already, its first planes are requested now,
            // and the dead jobs are filled while they fly.
            my_jobs = __builtin_amdgcn_readfirstlane(cnt[103]);
            NPL = bal_keep ? __builtin_amdgcn_readfirstlane(cnt[105]) : my_jobs * zs.PL;   // (TRIMMED JOBS: the sum of len + 8)
            nslots = NPL + kZD;
            if (!early) {
                npre = NPL < kZPre ? NPL : kZPre;
                for (int p = wave; p < 4 * npre; p += kW) dma_pass(p >> 2, p & 3, lane);
                if (tid >= 64 && tid < 128) cnt[32 + tid - 64] = (((tid - 64) & 15) < npre && !((zs.dbg & 1) && tid == 64)) ? 1 : 0;
            }
            // what a dead job's rounds would have stored, four values per thread and store: zero_round1 / zero_round2's
            // operations from e = + 0.0 on (the zero made opaque so that they are issued), for the rows and planes inside the grid
            int dead_rounds = 0;
            // (TRIMMED JOBS: the ranges are the dead jobs' whole segments and, under bal_keep, the two flanks [z0, a) and
            // [a + len, z1) of every live job -- item 2 k and 2 k + 1; an untrimmed job's flanks are empty)
            const int nflank = bal_keep ? 2 * my_jobs : 0;
#pragma unroll 1
            for (int it = 0; it < nflank + dealt - my_jobs; ++it) {
                const bool flank = it < nflank;
                const int k = flank ? it >> 1 : my_jobs + it - nflank;
                int4 jb = jobtab[k];
                int nz = zs.Z - jb.w < zs.LZ ? zs.Z - jb.w : zs.LZ;
                const int t = jb.z;
                if (bal) jb.z = 0;   // (one y tile; the field holds a | len << 8)
                if (flank) {
                    const int a = t & 255, e = a + (t >> 8);
                    if (it & 1) { nz = jb.w + nz - e; jb.w = e; }
                    else nz = a - jb.w;
                    if (nz <= 0) continue;
                }
                const int nx = zs.X - jb.y < kZTX ? zs.X - jb.y : kZTX;
                const int ny4 = (zs.Y - jb.z < TY ? zs.Y - jb.z : TY) >> 2;
                dead_rounds += nz * ((nx + kH - 1) / kH);
                if (!out) continue;
                OT* const tile = out + (size_t)jb.x * V;
#pragma unroll 1
                for (int i = tid; i < nz * (kZTX * 16); i += kNT) {
                    const int yq = i & 15, xr = (i >> 4) & (kZTX - 1), pz = i >> 7;
                    if (yq >= ny4 || xr >= nx) continue;
                    OT* const o = tile + (unsigned)(((jb.w + pz) * zs.X + jb.y + xr) * zs.Y + jb.z + 4 * yq);
                    float t[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                    asm volatile("" : "+v"(t[0]), "+v"(t[1]), "+v"(t[2]), "+v"(t[3]));
                    if (zs.head & 1) {
                        if constexpr (sizeof(OT) == 4) {
                            const float4 v = *reinterpret_cast<const float4*>(o);
                            t[0] += v.x; t[1] += v.y; t[2] += v.z; t[3] += v.w;
                        } else {
                            const double2 v = reinterpret_cast<const double2*>(o)[0], w = reinterpret_cast<const double2*>(o)[1];
                            t[0] += (float)v.x; t[1] += (float)v.y; t[2] += (float)w.x; t[3] += (float)w.y;
                        }
                    }
                    if (zs.head & 2) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) t[e] = relu_tanh(t[e]);
                    }
                    if constexpr (sizeof(OT) == 4) {
                        *reinterpret_cast<float4*>(o) = make_float4(t[0], t[1], t[2], t[3]);
                    } else {
                        reinterpret_cast<double2*>(o)[0] = make_double2((double)t[0], (double)t[1]);
                        reinterpret_cast<double2*>(o)[1] = make_double2((double)t[2], (double)t[3]);
                    }
                }
            }
            if (my_jobs == 0) {
                // no live job: the workgroup has filled everything it was dealt and requested nothing (npre = 0); its rounds
                // go to the device's count directly
                if (tid == 0) atomicAdd(&g_zwalk_rounds[1], (unsigned long long)(unsigned)dead_rounds);
                return;
            }
            if (wave == 0) n_skip = dead_rounds;
            if (!early) {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // (the first planes have landed: landed[] above says so)
                __syncthreads();
            }
        }
    }
    if constexpr (kLean) {
        if (tid == 0) {   // (for the device's plane counts, added with the round counts at the workgroup's end)
            cnt[106] = NPL;
            cnt[107] = my_jobs * zs.PL - NPL;
        }
    }
    SN_ST(4);

    bool healthy = true;
    const int ntickets = kTPS * nslots;
    auto claim = [&]() -> int {
        int t = 0;
        if (lane == 0) t = __hip_atomic_fetch_add(ticket_ctr, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        return __builtin_amdgcn_readfirstlane(t);
    };
    int pend = -1;   // index of the landed counter this wave owes a signal for (its last LDS-DMA pass), -1: none
    // HAND-OVER 1 (LDS-DMA -> fold pass, another wave): the issuing wave's s_waitcnt vmcnt(0) retires its LDS-DMA (vmcnt counts
    // in issue order; the data is in LDS when it decrements), THEN its ds_add_u32 publishes landed[pass][slot]; the fold's wave
    // sees the count in its dependency read and issues its ds_read of the raw rows behind that read (DS operations of a wave
    // execute in order).  [measured, tools/micro/ldsdma_handover.hip: 1.2e9 such hand-overs with the reader already
    // spinning, no stale word; with the add moved ahead of the wait, 3.0e6 stale words in 1.2e9]
    auto signal_passes = [&](int first) { lds_add_lane0<1>(&cnt[first], 1, lane); };

    int next = claim();
    for (int t = next; t < ntickets; t = next) {
        const unsigned long long tz0 = SN_ZNOW();
        next = claim();
        // per-lane constants of the ticket's bookkeeping (dependency-check roles, LDS-DMA lane, fold row) are recomputed from
        // an opaque copy of the lane id at every ticket: kept live through the rounds they were spilled, and a spill's reload
        // waits (vmcnt) for the wave's LDS-DMA and its epilogue stores
        int ln = lane;
        asm volatile("" : "+v"(ln));
        const int s = t >> kTShift, tk = t & (kTPS - 1);
        // !kLean: the round's table rows are requested here, a dependency check and two passes ahead of their use (tables, not
        // rings: nothing of the hand-over protocol; requested at the set-up itself their latency ate what the table saves)
        int4 LT, ST;
        if constexpr (!kLean) {
            LT = ltab[ln];
            ST = *reinterpret_cast<const int4*>(reinterpret_cast<const uint8_t*>(stab) + ((s - kZD) & 15) * 64 + (ln & 0x30));
        }
        const bool pass_ticket = kTPS <= 4 || (tk & 1) == 0;      // this ticket carries LDS-DMA / fold passes
        const int xr0 = kTPS == 8 ? tk >> 1 : tk;                 // ... pass xr0 of the plane
        const int sd = s + kZDD;
        const bool has_dma = pass_ticket && s >= kZD && sd < NPL;     // (planes below kZPre = kZD + kZDD: the prologue's)
        const bool has_fold = pass_ticket && s < NPL;
        const int sigma = s - kZD;
        int kr = 0, o = 0;
        bool has_round = false;
        if (sigma >= 0) {
            if constexpr (kLean) {
                // THE CURSOR: sigma < NPL (nslots = NPL + kZD), so the job it reaches is one of the table's live ones
                while (sigma >= sr_.end && sr_.next < dealt) {
                    job_step(jr, sr_);
                    if (out) ob = out + (size_t)jr.b * V;
                }
                o = sigma - sr_.s0;
                has_round = o < sr_.len;
            } else {
                kr = (int)__umulhi((unsigned)sigma, zs.pl_magic);
                o = sigma - kr * zs.PL;
                has_round = o < zs.LZ;
            }
        }
        // a pass this wave requested in an earlier ticket and has not reported yet (that ticket had no round to hide the
        // wait behind).  Reported before anything is waited for: this ticket's own dependencies may lead back to it
        // ([measured] partial columns, whose skipped rounds leave the report pending: 4M-spin timeouts, 0.45 s per launch).
        if (pend >= 0) {
            asm volatile("; @zw:wait1\n\ts_waitcnt vmcnt(0)" ::: "memory");
            signal_passes(pend);
            pend = -1;
        }
        SN_ZT(0, tz0);
        const unsigned long long tz1 = SN_ZNOW();
        int midx;   // lanes 0..8: ring slot of plane sigma + i (the dependency check's counter index)
        // ---- everything this ticket depends on, in one LDS read: lane roles
        //   0..8   folded[plane sigma + i]   (round: its nine planes)           16..24  read[slot s - 14 + i]  (fold: the readers
        //   32..   landed[plane s][pass]     (fold: its raw rows)                        of the plane it overwrites)
        //   40     folded[plane sd - 16]     (DMA: the raw slot it overwrites has been folded)
        {
            const int4 role = chk[ln];
            const int have = (has_round ? 1 : 0) | (has_fold ? 2 : 0) | (has_dma ? 4 : 0) | 8;
            const int v = s + role.x;
            const int idx = ((v & 15) | role.y) + (role.z & (xr0 * 16));   // (bits 4, 5 of role.z: the landed counter of pass xr0)
            const int expect = ((role.z & have) && v >= 0) ? (((v >> 4) + 1) << role.w) : 0;
            midx = idx;
            int spins = 0;
            while (true) {
                // (an LDS read, spelled in its address space: through a generic volatile pointer hipcc emits a FLAT load with
                // system-scope coherence bits and waits vmcnt(0) for it -- i.e. for the wave's LDS-DMA and epilogue stores)
                const int seen = reinterpret_cast<const volatile __attribute__((address_space(3))) int*>(
                    (__attribute__((address_space(3))) int*)cnt)[idx];
                if (__builtin_amdgcn_ballot_w64(seen < expect) == 0ull) break;
                // cannot happen (every dependency is an earlier ticket); never hang the GPU.  Every 64th spin also looks at the
                // workgroup's give-up flag, so that one wave's give-up ends the others' waits at once, not 4M spins later each.
                if (++spins > kSpinMax ||
                    ((spins & 63) == 0 &&
                     reinterpret_cast<const volatile __attribute__((address_space(3))) int*>((__attribute__((address_space(3))) int*)cnt)[98] != 0)) {
                    healthy = false;
                    break;
                }
                __builtin_amdgcn_s_sleep(2);
            }
            // HAND-OVERS 1..4, consumer side: nothing below -- no ds_read of ring or raw data, no LDS-DMA, no store to the rings
            // -- may move above this point.  The counter read is volatile and the wave has WAITED for its value (the ballot
            // needs it); the clobber keeps hipcc's plain LDS accesses behind it (audited in the ISA).
            asm volatile("; @zw:spin_exit" ::: "memory");
        }
        if (!healthy) {
            // a dependency never arrived (this wave's spin gave up, or another wave's did): stop taking tickets; the code
            // behind the loop poisons the workgroup's outputs.  The status is latched HERE, by the wave that saw it first.
            if (lane == 0) {
                reinterpret_cast<volatile __attribute__((address_space(3))) int*>((__attribute__((address_space(3))) int*)cnt)[98] = 1;
                sn::sticky_latch(zs.sticky, 1, (int)blockIdx.x, t);
            }
            break;
        }
        SN_ZT(1, tz1);
        const unsigned long long tz2 = SN_ZNOW();
        // the row masks of the ticket's nine planes (lanes 0..8; the other lanes read whatever their counter index points at
        // in the words behind the masks and are cut from the ballot): guarded data, requested behind the spin exit and ahead
        // of the ticket's passes, whose own LDS waits cover its latency.  Every ticket reads them (a ticket without a round
        // drops the value) and every read[] report waits for the read's return first (`@zw:wait3`).
        const uint32_t rmask = reinterpret_cast<const volatile __attribute__((address_space(3))) uint32_t*>(
            (__attribute__((address_space(3))) uint32_t*)rowmask)[midx];
        if (has_dma) {
            dma_pass(sd, xr0, ln);
            pend = 32 + xr0 * 16 + (sd & 15);
        }
        if (has_fold) {
            fold_pass(s, xr0, ln);
            // HAND-OVER 2 (fold pass -> rounds, other waves): ds_write_b128 + ds_write_b32 of the folded rows, then ds_add_u32 on
            // folded[slot] -- one wave's DS operations reach the LDS in order ([measured] the register-staged mode of
            // tools/micro/ldsdma_handover.hip: ds_write_b128 -> ds_add_u32, reader spinning: no stale word in 3e8), and the
            // `memory` clobber of the asm keeps hipcc from moving the stores below it (audited in the ISA).
            lds_add_lane0<2>(&cnt[s & 15], 1, lane);
        }
        SN_ZT(2, tz2);
        if (!has_round) {
            asm volatile("; @zw:wait3\n\ts_waitcnt lgkmcnt(0)" ::: "memory");
            lds_add_lane0<3>(&cnt[16 + (s & 15)], 1, lane);
            continue;
        }
        const unsigned long long tz3 = SN_ZNOW();
        if constexpr (!kLean) job_fetch(jr, kr);   // (kLean: the cursor above)
        const int gz = jr.zs + o;
        const int lx = kH * kR * tk;   // the ticket's first x-row
        int rows_left = 0, nvalid = 0;   // rounds of this ticket that lie inside the grid (x-rows past X end the ticket early)
        if (gz >= zs.Z || jr.x0 + lx >= zs.X) {   // (a last segment shorter than LZ; x-rows past the grid)
            asm volatile("; @zw:wait3\n\ts_waitcnt lgkmcnt(0)" ::: "memory");   // (the mask read: nothing else was read)
            lds_add_lane0<3>(&cnt[16 + (s & 15)], 1, lane);
            continue;
        }
        if constexpr (kLean) {
            rows_left = zs.X - (jr.x0 + lx);
            nvalid = rows_left >= kH * kR ? kR : (rows_left + kH - 1) / kH;
        }
        // THE TICKET'S VERDICT FIRST (round 7): one window over all its rounds -- rows lx .. lx + kH kR + 7 of the nine planes,
        // the union of the rounds' windows -- decides whether anything of the round set-up below is needed.  On the C2 batch
        // 72 % of the rounds are empty and most empty rounds share their ticket with another: such a ticket pays the report,
        // one row address and its stores, nothing else.
        if (kLean && can_skip) {
            const uint32_t ub = zwindow_mask<kH * kR>(kH * kR == 2 ? (tk & 1) * 2 : (tk & 3), kH * kR == 2 ? tk >> 1 : tk >> 2);
            if (((uint32_t)__builtin_amdgcn_ballot_w64((rmask & ub) != 0u) & 0x1ffu) == 0u) {
                // every round of the ticket is empty.  The read[] report stays where an empty round's was (HAND-OVER 3): the
                // mask read has returned (the verdict needed it), nothing else was read.
                asm volatile("; @zw:wait3\n\ts_waitcnt lgkmcnt(0)" ::: "memory");
                lds_add_lane0<3>(&cnt[16 + (s & 15)], 1, lane);
                n_skip += nvalid;
                // what the rounds would store for all-zero accumulators (zero_round1 / zero_round2 above).  Under head & 1 (load,
                // add, activate) that is those functions' own; without head & 1 the value is relu_tanh(+ 0.0) or + 0.0 itself --
                // both are + 0.0 bits (relu_tanh: 0 < v fails, v != v fails: the constant 0.0f) -- and is stored as that constant:
                // one row address per ticket, no evaluation per round.
                if (ob && (zs.head & 1)) {
                    TileCoord c;
                    c.b = 0; c.x0 = jr.x0; c.y0 = jr.y0; c.z0 = gz;   // (b: in the base)
                    const int n = ln & 15, q = ln >> 4;
#pragma unroll 1
                    for (int rr = 0; rr < nvalid; ++rr) {
                        if constexpr (kH == 2) zero_round2<OT>(zs, c, lx + rr * kH, n, q, act, ob, V);
                        else zero_round1<OT>(zs, c, lx + rr * kH, n, q, 4 * n + q, act, ob, V);
                    }
                }
                if (ob && !(zs.head & 1)) {
                    OT* const row = ob + (unsigned)((gz * zs.X + jr.x0 + lx) * zs.Y);   // (scalar; y = 0 of the ticket's first row)
                    float z0 = 0.0f;
                    asm volatile("" : "+v"(z0));   // (made here: as a loop invariant the constant pair was kept in registers and spilled)
                    const OT zero = (OT)z0;
                    if (kH * kR == 2 && rows_left >= 2 && zs.nyt == 1) {
                        // both rows lie in the grid and one y tile spans Y: 2 Y consecutive values, two per lane
                        if (ln < zs.Y) {
                            OT* const o2 = row + 2u * (unsigned)ln;
                            if constexpr (sizeof(OT) == 4) *reinterpret_cast<float2*>(o2) = make_float2(zero, zero);
                            else *reinterpret_cast<double2*>(o2) = make_double2(zero, zero);
                        }
                    } else {
                        const int gy = jr.y0 + ln;
                        if (gy < zs.Y) {
                            row[(unsigned)gy] = zero;
                            if (kH * kR == 2 && rows_left >= 2) row[(unsigned)(zs.Y + gy)] = zero;
                        }
                    }
                }
                SN_ZT(6, tz0);
                continue;
            }
        }
        // ---- the round set-up: only for a ticket that runs a round (or may not skip)
        TileCoord c;
        c.b = kLean ? 0 : jr.b; c.x0 = jr.x0; c.y0 = jr.y0; c.z0 = gz;   // (kLean: b is in the base ob)
        OT* const oq = kLean ? ob : out;
        // kLean: the rounds' table rows (tables, not rings: nothing of the hand-over protocol); their latency hides behind the
        // scalar part of the set-up and the per-round masks
        if constexpr (kLean) {
            LT = ltab[ln];
            ST = *reinterpret_cast<const int4*>(reinterpret_cast<const uint8_t*>(stab) + ((s - kZD) & 15) * 64 + (ln & 0x30));
        }
        // (the rounds' per-lane constants, likewise from an opaque lane id: see the top of the ticket)
        const int lr = ln;
        const int n16 = LT.x, q256 = LT.y;
        __builtin_assume((n16 & 15) == 0 && (q256 & 255) == 0);
        const int n4 = n16 >> 2, q64 = q256 >> 2;
        const int n = n16 >> 4, q = q256 >> 8;
        // per-lane ring addresses (LDS byte addresses; the uniform parts pinned to scalar registers): the lane group's
        // planes dz = 2 q, 2 q + 1 (from the table), and plane 8
        using lds_cp = const __attribute__((address_space(3))) uint8_t*;
        auto at = [&](int a) { return (const uint8_t*)(lds_cp)(uintptr_t)(uint32_t)a; };
        const int s8 = (sigma + 8) & 15;
        const int uq = __builtin_amdgcn_readfirstlane(lx * kZYqRow), uc = __builtin_amdgcn_readfirstlane(lx * kZYcRow);
        const int u8q = __builtin_amdgcn_readfirstlane((int)(uint32_t)(uintptr_t)(lds_cp)Yq + s8 * kZYqPlane + lx * kZYqRow);
        const int u8c = __builtin_amdgcn_readfirstlane((int)(uint32_t)(uintptr_t)(lds_cp)Yc + s8 * kZYcPlane + lx * kZYcRow);
        const uint8_t* yqA = at(ST.x + n16 + uq);
        const uint8_t* yqB = at(ST.z + n16 + uq);
        const uint8_t* yq8 = at(u8q + n16);
        const uint8_t* ycA = at(ST.y + n4 + uc);
        const uint8_t* ycB = at(ST.w + n4 + uc);
        const uint8_t* yc8 = at(u8c + n4);

        // operand unit (slot, x-row h): the folded quads of halo rows h1 (r[0..3], centre r[4]) and h2 (r[5..8], r[9])
        auto load_unit = [&](auto SLOT, auto HC, uint32_t (&r)[10]) {
            constexpr int slot = decltype(SLOT)::value, h = decltype(HC)::value;
            constexpr bool single = fold_slot_single(slot / kFoldRows, slot % kFoldRows);
            const uint8_t *q1, *q2, *c1, *c2;
            if constexpr (slot == 8) {
                q1 = yq8 + (h + 4) * kZYqRow; c1 = yc8 + (h + 4) * kZYcRow;
                q2 = q1; c2 = c1;
            } else if constexpr (slot == 11) {
                q1 = yq8 + h * kZYqRow + q256; c1 = yc8 + h * kZYcRow + q64;               // rows h + q and h + 8 - q
                q2 = yq8 + (h + 8) * kZYqRow - q256; c2 = yc8 + (h + 8) * kZYcRow - q64;
            } else {
                constexpr int dx = fold_slot_dx(slot);
                const uint8_t* bq = fold_slot_a(slot) ? yqB : yqA;
                const uint8_t* bc = fold_slot_a(slot) ? ycB : ycA;
                q1 = bq + (h + dx) * kZYqRow; c1 = bc + (h + dx) * kZYcRow;          // (immediates of the reads)
                q2 = bq + (h + 8 - dx) * kZYqRow; c2 = bc + (h + 8 - dx) * kZYcRow;
            }
            const uint4 a = *reinterpret_cast<const uint4*>(q1);
            r[0] = a.x; r[1] = a.y; r[2] = a.z; r[3] = a.w;
            r[4] = *reinterpret_cast<const uint32_t*>(c1);
            if constexpr (!single) {
                const uint4 b = *reinterpret_cast<const uint4*>(q2);
                r[5] = b.x; r[6] = b.y; r[7] = b.z; r[8] = b.w;
                r[9] = *reinterpret_cast<const uint32_t*>(c2);
            }
        };
        // the x fold: component J of the four residues' operand quads, and the summed centre dword
        auto fold_unit = [&](const uint32_t (&r)[10], auto SLOT, i32x4 (&X)[4], uint32_t& centre) {
            constexpr int slot = decltype(SLOT)::value, J = slot % kFoldRows;
            constexpr bool single = fold_slot_single(slot / kFoldRows, J);
            if constexpr (single) {
                X[0][J] = (int)r[0]; X[1][J] = (int)r[1]; X[2][J] = (int)r[2]; X[3][J] = (int)r[3];
                centre = r[4];
            } else {
                X[0][J] = (int)(r[0] + r[5]); X[1][J] = (int)(r[1] + r[6]);
                X[2][J] = (int)(r[2] + r[7]); X[3][J] = (int)(r[3] + r[8]);
                centre = r[4] + r[9];
            }
        };
        auto centres = [&](uint32_t c0, uint32_t c1, uint32_t c2, i32x4 (&X)[4]) {
            uint32_t ov[4];
            transpose3(c0, c1, c2, ov);
#pragma unroll
            for (int r = 0; r < 4; ++r) X[r][3] = (int)ov[r];
        };
        if constexpr (!kLean) {
            rows_left = zs.X - (c.x0 + lx);
            nvalid = rows_left >= kH * kR ? kR : (rows_left + kH - 1) / kH;
        }
        // which of the ticket's rounds have a set voxel in their window (wave-uniform): rows lx + rr kH .. + kH + 7 of the
        // nine planes, as bits of the masks' layout (byte xr, bit q).  (kR = 1: the ticket's verdict above was the round's.)
        uint32_t hits[kR];   // lanes 0..8 with a row bit inside the window of round rr (scalar)
#pragma unroll
        for (int rr = 0; rr < kR; ++rr) {
            if (kLean && kR == 1) { hits[rr] = 1u; continue; }
            uint32_t wb;
            if constexpr (kLean) {
                wb = zwindow_mask<kH>((tk & 1) * 2 + rr, tk >> 1);   // (kH = 1, kR = 2: row 2 tk + rr)
            } else {
                const uint32_t w = ((1u << (8 + kH)) - 1u) << (lx + rr * kH);
                wb = (w & 0xfu) | ((w & 0xf0u) << 4) | ((w & 0xf00u) << 8) | ((w & 0xf000u) << 12);
            }
            asm("" : "+s"(wb));   // (one scalar operand: v_and + v_cmp per round)
            hits[rr] = can_skip ? ((uint32_t)__builtin_amdgcn_ballot_w64((rmask & wb) != 0u) & 0x1ffu) : 1u;
        }
        // The ticket's rounds run as a LOOP (not unrolled: one copy of the round's code, one round's registers -- [measured]
        // two unrolled rounds spilled 27 reloads into the loop and were no faster than one round per ticket); the six ring
        // addresses advance by kH rows per round.
#pragma unroll 1
        for (int rr = 0; rr < nvalid; ++rr) {
            if ((kR == 1 || rr == 0 ? hits[0] : hits[kR - 1]) == 0u) {
                // an empty window: no operand read, no weight read, no MFMA.  The ticket's read[] report stays where it is
                // (HAND-OVER 3): the mask read has returned (the verdict needed it), and a round of this ticket that ran
                // has waited for its ring reads before its last MFMA step's operands were formed.
                if (rr == nvalid - 1) {
                    asm volatile("; @zw:wait3\n\ts_waitcnt lgkmcnt(0)" ::: "memory");
                    lds_add_lane0<3>(&cnt[16 + (s & 15)], 1, lane);
                }
                if constexpr (kH == 2) zero_round2<OT>(zs, c, lx + rr * kH, n, q, act, oq, V);
                else zero_round1<OT>(zs, c, lx + rr * kH, n, q, LT.z, act, oq, V);
                ++n_skip;
                yqA += kH * kZYqRow; yqB += kH * kZYqRow; yq8 += kH * kZYqRow;
                ycA += kH * kZYcRow; ycB += kH * kZYcRow; yc8 += kH * kZYcRow;
                continue;
            }
            ++n_run;
            constexpr int ro = 0;
            // A step has 3 kH operand units u = (row j = u / kH, x-row h = u % kH) and kH centre transposes: 4 kH pieces,
            // built behind the 4 kH MFMA groups of the step before; unit u's quads are requested kAhead pieces before its fold.
            constexpr int kNU = 3 * kH, kNP = 4 * kH;
            uint32_t praw[kNU][10], pcen[3][kH];
            auto pipe_load = [&](auto ST, auto UC) {
                constexpr int st = decltype(ST)::value, u = decltype(UC)::value;
                load_unit(std::integral_constant<int, st * kFoldRows + u / kH>{}, std::integral_constant<int, u % kH + ro>{}, praw[u]);
            };
            constexpr int kAhead = SN_I8Z_AHEAD;
            auto pipe_piece = [&](auto ST, auto PC, i32x4 (&X)[kH][4], auto NST) {
                constexpr int st = decltype(ST)::value, piece = decltype(PC)::value, nst = decltype(NST)::value;
                if constexpr (piece < kNU) {
                    constexpr int j = piece / kH, h = piece % kH;
                    fold_unit(praw[piece], std::integral_constant<int, st * kFoldRows + j>{}, X[h], pcen[j][h]);
                } else {
                    constexpr int h = piece - kNU;
                    centres(pcen[0][h], pcen[1][h], pcen[2][h], X[h]);
                }
                if constexpr (piece + kAhead < kNU) pipe_load(ST, std::integral_constant<int, piece + kAhead>{});
                else if constexpr (piece >= kNP - kAhead && nst >= 0 && piece - (kNP - kAhead) < kNU)
                    pipe_load(std::integral_constant<int, (nst < 0 ? 0 : nst)>{}, std::integral_constant<int, piece - (kNP - kAhead)>{});
            };
            constexpr std::integral_constant<int, 0> S0{};
            constexpr std::integral_constant<int, 1> S1{};
            constexpr std::integral_constant<int, 2> S2{};
            constexpr std::integral_constant<int, 3> S3{};
            constexpr std::integral_constant<int, -1> SNone{};

            i32x4 acc[3][kNVz];
            auto load_w = [&](int st, i32x4 (&w)[3]) {
#pragma unroll
                for (int d = 0; d < 3; ++d) {
                    const uint4 u = Wd[(st * 3 + d) * 64 + lr];
                    w[d] = i32x4{(int)u.x, (int)u.y, (int)u.z, (int)u.w};
                }
            };
            auto mma_tile = [&](const i32x4 (&w)[3], const i32x4& xv, int v, bool first) {
#pragma unroll
                for (int d = 0; d < 3; ++d)
                    acc[d][v] = __builtin_amdgcn_mfma_i32_16x16x64_i8(w[d], xv, first ? i32x4{0, 0, 0, 0} : acc[d][v], 0, 0, 0);
            };
            auto mma_step = [&](const i32x4 (&w)[3], const i32x4 (&X)[kH][4], bool first, auto&& work) {
                auto group = [&](auto VC) {
                    constexpr int v = decltype(VC)::value, h = v >> 2, r = v & 3;
                    mma_tile(w, X[h][r], v, first);
                    __builtin_amdgcn_sched_barrier(0);
                    work(VC);
                    __builtin_amdgcn_sched_barrier(0);
                };
                group(std::integral_constant<int, 0>{}); group(std::integral_constant<int, 1>{});
                group(std::integral_constant<int, 2>{}); group(std::integral_constant<int, 3>{});
                if constexpr (kH == 2) {
                    group(std::integral_constant<int, 4>{}); group(std::integral_constant<int, 5>{});
                    group(std::integral_constant<int, 6>{}); group(std::integral_constant<int, 7>{});
                }
            };
            i32x4 Xa[kH][4], Xb[kH][4];
            i32x4 wa[3], wb[3];
            // step 0, un-pipelined: its units, then their folds
            load_w(0, wa);
            {
                auto all_units = [&](auto&& f) {
                    f(std::integral_constant<int, 0>{}); f(std::integral_constant<int, 1>{}); f(std::integral_constant<int, 2>{});
                    if constexpr (kH == 2) {
                        f(std::integral_constant<int, 3>{}); f(std::integral_constant<int, 4>{}); f(std::integral_constant<int, 5>{});
                    }
                };
                all_units([&](auto U) { pipe_load(S0, U); });
                all_units([&](auto U) {
                    constexpr int u = decltype(U)::value;
                    fold_unit(praw[u], std::integral_constant<int, u / kH>{}, Xa[u % kH], pcen[u / kH][u % kH]);
                });
#pragma unroll
                for (int h = 0; h < kH; ++h) centres(pcen[0][h], pcen[1][h], pcen[2][h], Xa[h]);
                // (the units a pipelined step expects to find requested when it starts)
                auto first_ahead = [&](auto U) {
                    constexpr int u = decltype(U)::value;
                    if constexpr (u < kAhead && u < kNU) pipe_load(S1, U);
                };
                first_ahead(std::integral_constant<int, 0>{}); first_ahead(std::integral_constant<int, 1>{});
                first_ahead(std::integral_constant<int, 2>{}); first_ahead(std::integral_constant<int, 3>{});
            }
            load_w(1, wb);
            __builtin_amdgcn_sched_barrier(0);
            if (rr == 0) SN_ZT(3, tz3);
            const unsigned long long tz4 = SN_ZNOW();
            mma_step(wa, Xa, true, [&](auto v) { pipe_piece(S1, v, Xb, S2); });
            load_w(2, wa);
            __builtin_amdgcn_sched_barrier(0);
            mma_step(wb, Xb, false, [&](auto v) { pipe_piece(S2, v, Xa, S3); });
            load_w(3, wb);
            __builtin_amdgcn_sched_barrier(0);
            mma_step(wa, Xa, false, [&](auto v) { pipe_piece(S3, v, Xb, SNone); });
            __builtin_amdgcn_sched_barrier(0);
            // HAND-OVER 3 (rounds -> the fold that overwrites their planes, another wave): every ring read of this ticket has
            // returned (s_waitcnt lgkmcnt(0): the last unit's quads are in registers), THEN ds_add_u32 on read[slot]; the fold
            // pass checks read[s - 13 .. s - 5] before its first ds_write.  (HAND-OVER 4, fold pass -> the LDS-DMA that
            // overwrites its raw rows: the fold's ds_reads of the raw rows have returned before its ds_writes are issued --
            // they carry the data -- and folded[slot] is added behind those; the LDS-DMA's ticket checks folded[sd - 16].)
            if (rr == nvalid - 1) {   // the ticket's last round
                asm volatile("; @zw:wait3\n\ts_waitcnt lgkmcnt(0)" ::: "memory");
                lds_add_lane0<3>(&cnt[16 + (s & 15)], 1, lane);
            }
            mma_step(wb, Xb, false, [](auto) {});
            if (pend >= 0) {
                asm volatile("; @zw:wait1\n\ts_waitcnt vmcnt(0)" ::: "memory");   // (requested a round ago: long since landed)
                signal_passes(pend);
                pend = -1;
            }
            SN_ZT(4, tz4);
            const unsigned long long tz5 = SN_ZNOW();
            if constexpr (kH == 2 && kLean) {
                // (n and q again from the lane id: kept live through the MFMA steps of this 256-register shape they were spilled)
                int le = lr;
                asm volatile("" : "+v"(le));
                finish_round<OT>(zs, c, 0, lx + rr * kH, le & 15, le >> 4, acc, scale, lamsc, lamhi, act, oq, V);
            } else if constexpr (kH == 2) finish_round<OT>(zs, c, 0, lx + rr * kH, n, q, acc, scale, lamsc, lamhi, act, oq, V);
            else finish_round1<OT>(zs, c, lx + rr * kH, n, q, LT.z, LT.w, acc, scale, lamsc, lamhi, act, oq, V);
            SN_ZT(5, tz5);
            yqA += kH * kZYqRow; yqB += kH * kZYqRow; yq8 += kH * kZYqRow;
            ycA += kH * kZYcRow; ycB += kH * kZYcRow; yc8 += kH * kZYcRow;
        }
        SN_ZT(6, tz0);
    }
    SN_ST(5);
    if (pend >= 0) {
        asm volatile("; @zw:wait1\n\ts_waitcnt vmcnt(0)" ::: "memory");
        signal_passes(pend);
    }
    // ---- round counts: every wave adds its own to the workgroup's LDS words, the last one to do so adds the sums to the
    // device's (one pair of global atomics per workgroup; a wave's DS operations reach the LDS in order)
    if (lane == 0) {
        const uint32_t a = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) int*)(cnt + 100);
        asm volatile("ds_add_u32 %0, %1\n\tds_add_u32 %0, %2 offset:4" ::"v"(a), "v"(n_run), "v"(n_skip) : "memory");
        if (atomicInc(reinterpret_cast<unsigned*>(cnt + 102), 0xffffffffu) == (unsigned)kW - 1u) {
            const volatile __attribute__((address_space(3))) int* tot = (__attribute__((address_space(3))) int*)cnt;
            atomicAdd(&g_zwalk_rounds[0], (unsigned long long)(unsigned)tot[100]);
            atomicAdd(&g_zwalk_rounds[1], (unsigned long long)(unsigned)tot[101]);
            if constexpr (kLean) {
                atomicAdd(&g_zwalk_planes[0], (unsigned long long)(unsigned)tot[106]);
                atomicAdd(&g_zwalk_planes[1], (unsigned long long)(unsigned)tot[107]);
            }
        }
    }
    // ---- a wave of this workgroup gave up: nothing the workgroup wrote can be trusted.  Every wave that is still alive gets
    // here (the flag ends every spin; a barrier does not wait for waves that have ended), its own stores are out (vmcnt),
    // and together they overwrite the workgroup's outputs with NaN.  sn_conv_i8_spin_timeouts counts the waves.
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (reinterpret_cast<const volatile __attribute__((address_space(3))) int*>((__attribute__((address_space(3))) int*)cnt)[98] != 0) {
        __syncthreads();
        poison_jobs();
        if (!healthy && lane == 0) atomicAdd(&g_fold_counts[3], 1ull);
    }
}

// The launch enqueued behind the walk: does nothing unless the walk's verdict (above) sent the job on -- then the unfolded
// int8 body (bank not symmetric in x and y) or the fp32 form (quantisation bound over the tolerance; also where the unfolded
// body's own guard sends it) runs in place, with the same code, hence the same bits, as sn_conv_bank's own kernels.
template <typename OT>
__global__ __launch_bounds__(kThreads) void conv_i8_fallback_kernel(const uint8_t* __restrict__ x,
                                                                    const float* __restrict__ bank,
                                                                    const float* __restrict__ lambdas,
                                                                    const int32_t* __restrict__ route, Shape s4,
                                                                    fp32k::ConvShape cs, OT* __restrict__ act,
                                                                    OT* __restrict__ out) {
    if (!cs.gate.pass()) return;
    const int verdict = *route;
    if (verdict <= 0) return;   // 0: the walk served the launch;  -1: no walk ran behind this preparation (a gated launch)
    bool to_fp32 = verdict == 1;
    if (verdict == 2) {
        to_fp32 = conv_occ_i8s_body<OT, 10, 6, 1>(x, bank, lambdas, s4, act, out);   // (s4.route == nullptr: the verdict stays)
        if (to_fp32) __syncthreads();
    }
    if (to_fp32) fp32k::conv_bank_body<uint8_t, OT, false>(x, bank, lambdas, cs, act, out);
}

size_t lds_bytes_zwalk() {
    return (size_t)kFoldSteps * 3 * 64 * 16 + (size_t)kZMaxJobs * 16 + 64 * 4 + 128 + 128 * 4 + 64 * 16 + 2 * 64 * 16 +
           32 * 4 + (size_t)kZRing * (kZRawPlane + kZYcPlane + kZYqPlane) + 16;
}

// u / d == mulhi(u, magic) for all 0 <= u <= umax?  (magic = floor(2^32 / d) + 1; checked exhaustively: umax is small)
bool division_magic(unsigned d, unsigned umax, unsigned& magic) {
    magic = (unsigned)((((unsigned long long)1 << 32) / d) + 1ull);
    for (unsigned u = 0; u <= umax; ++u)
        if ((unsigned)(((unsigned long long)u * magic) >> 32) != u / d) return false;
    return true;
}
