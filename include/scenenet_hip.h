/*
 * scenenet_hip.h -- C ABI of the MI355X-native SCENE-Net GENEO hot path (forward, and the training rows of SURVEY 8f).
 *
 * The reference (dlavado/scene-net) is pure Python and has no FFI layer; its
 * "operator API" for this path is a set of Python classes/functions.  Each
 * entry point below names the reference interface it replaces (file:line,
 * relative to the reference tree).  INTEGRATION.md shows the ctypes stub a
 * maintainer adds on the reference side.
 *
 * Conventions
 *   - plain `extern "C"`, no torch / C++ types in any signature;
 *   - every pointer is a caller-allocated DEVICE pointer (e.g. tensor.data_ptr())
 *     unless the parameter name ends in `_host`;
 *   - `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream);
 *     every call only enqueues work on it (no allocation, no sync, graph-capturable; the only process state is a
 *     cache of per-kernel LDS attributes and, with the opt-in "conv_skip_empty_tiles", a device ring of ticket
 *     counters allocated once);
 *   - return value: 0 = SN_OK, negative = sn_status; sn_last_error() gives the
 *     message of the calling thread's last failure;
 *   - grids are [B, C, Z, X, Y] row-major, y fastest (utils/voxelization.py:193);
 *     GENEO kernels are [G, kz, kx, ky] row-major.
 */
#ifndef SCENENET_HIP_H
#define SCENENET_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* sn_stream_t;

typedef enum {
    SN_OK = 0,
    SN_ERR_INVALID_ARG = -1,   /* null pointer, non-positive extent, bad enum        */
    SN_ERR_UNSUPPORTED = -2,   /* shape outside what the kernels are built for       */
    SN_ERR_LAUNCH = -3,        /* hipGetLastError() after a launch                   */
    SN_ERR_NO_DEVICE = -4,     /* no gfx950 device / HIP runtime unusable            */
    SN_ERR_DEVICE_STATUS = -5  /* a kernel latched the sticky status: sn_device_status */
} sn_status;

/* SN_BF16: bfloat16 STORAGE of activations / their gradients in the training path (reference: `precision: 16`,
 * experiments/scenenet_ts40k/defaults_config.yml:83-84): accepted as out_dtype of sn_conv_fused, as pred / grad
 * dtype of sn_loss_forward / sn_loss_backward and as the gradient dtype of sn_conv_corr_t; every sum stays fp32 / fp64.
 * SN_OCC8: uint8 grid whose values are all 0 or 1 (binary occupancy, torch.bool) -- lets sn_conv_bank use the
 * int8 matrix cores.  SN_U8 is a general 0..255 byte grid.
 * SN_I32: int32 labels (torch.int, what `y.to(torch.int)` gives): accepted as the target of sn_binary_stats only;
 * every other entry rejects it. */
typedef enum { SN_F32 = 0, SN_F64 = 1, SN_U8 = 2, SN_OCC8 = 3, SN_BF16 = 4, SN_I32 = 5 } sn_dtype;

/* GENEO kinds: 0-2 = cylinderv2 / arrow / negSpherev2 of SceneNet (core/models/SCENE_Net.py:259-272);
 * 3-5 = cylinder_kernel / cone_kernel / neg_sphere_kernel of the v1 module SCENE_Net (SCENE_Net.py:158-170). */
typedef enum {
    SN_GENEO_CY = 0, SN_GENEO_CONE = 1, SN_GENEO_NEG = 2,
    SN_GENEO_CY_V1 = 3, SN_GENEO_CONE_V1 = 4, SN_GENEO_NEG_V1 = 5
} sn_geneo_kind;

/* Parameter slots of one GENEO: params[g * SN_NPARAM + slot] (fp32). */
enum {
    SN_P_RADIUS = 0,      /* cy, cone, neg : cylinder.py:55, arrow.py:78, neg_sphere.py:62 */
    SN_P_SIGMA = 1,       /* cy, cone, neg : default 1                                      */
    SN_P_APEX = 2,        /* cone          : truncated to int, arrow.py:235                 */
    SN_P_CONE_RADIUS = 3, /* cone          : arrow.py:84-87                                 */
    SN_P_CONE_INC = 4,    /* cone          : clamped to [0, 0.499], arrow.py:244            */
    SN_P_NEG_FACTOR = 5,  /* neg           : neg_sphere.py:63                               */
    SN_NPARAM = 8
};

int sn_version(void);
/* Allocates the current device's pool of flag / ticket words (20 KB) now -- the only allocation the library ever makes.
 * Optional: the first int8 launch on a device does it too, but that launch must then not be inside a stream capture
 * (hipMalloc / hipMemset are illegal there).  Launches made while their stream is capturing draw words that are never
 * handed out again, so a captured graph owns its flags (see csrc/cabi.hip). */
int sn_prepare_device(void);
/* The sticky device status (round 4).  A kernel that cannot keep its contract does not return plausible numbers: it
 * overwrites what it owns with NaN and latches a status in host-pinned words of its device --
 *   1  a dependency spin of the z-walk contraction gave up (sn_conv_bank_prepared[_served]);
 *   2  sn_conv_bank_prepared_served was called for a bank whose verdict is NOT "served" (a stale cached verdict);
 *   3  a hand-over spin of an int8 tile kernel gave up (sn_conv_bank, x_dtype SN_OCC8 / SN_U8)
 * -- and from then on EVERY sn_* entry that launches work fails with SN_ERR_DEVICE_STATUS (sn_last_error() says which code,
 * which workgroup) until sn_device_status_clear().  Looking at the words is a host memory read: no synchronisation, nothing
 * on the launch path.  sn_device_status: *code = 0 when healthy; detail2 (nullable) = {workgroup, ticket | verdict}.
 * sn_device_status_clear synchronises the device first.  The reference has no counterpart (its conv3d cannot fail this
 * way); this is the error behaviour of the hand-written path. */
int sn_device_status(int* code, int* detail2);
int sn_device_status_clear(void);
/* Diagnostics: how many sn_conv_bank launches (this device, this process) the folded int8 kernel served [0], declined
 * because the bank was not symmetric in x and y [1], and handed to the fp32 kernel because the quantisation bound
 * exceeded the tolerance [2].  Synchronises the device.  (No reference counterpart.) */
int sn_conv_i8_path_counts(unsigned long long* counts3);
const char* sn_last_error(void);

/* Number of gfx950 devices visible (0 when none); never throws. */
int sn_device_count(void);

/* Process-wide options (csrc/cabi.hip keeps them in one table, in this order).  A switch stores any value != 0 as 1; every
 * other option takes the range given with it.  sn_set_option returns SN_ERR_INVALID_ARG for a null or unknown name or a
 * value out of range (and changes nothing); sn_get_option returns -1 for a null or unknown name.  An option listed with an
 * environment variable reads it ONCE, the first time the option is looked at (never per call); only its first character
 * counts, '1' giving the value shown; an sn_set_option before that first look wins, and the variable is then never read.
 *   "conv_skip_empty_tiles" (switch, default 0): sn_conv_bank on SN_OCC8 input skips the MFMA steps of workgroup tiles whose
 *       halo holds no set voxel (their response is exactly 0 for every kernel).  Output unchanged; run time becomes
 *       data dependent, so benchmarks quote it separately from the dense figure.
 *   "conv_i8_tolerance_ppb" (>= 0, default 90000 = 9e-5): the int8 kernels (sn_conv_bank / sn_conv_fused / sn_forward_auto on
 *       binary occupancy) quantise the weights to 24-bit fixed point and compute, on the device, the exact worst case
 *       of the resulting activation error over all binary inputs.  A bank whose bound exceeds value * 1e-9 is computed
 *       by the fp32 kernel instead (decided on the device, no host synchronisation).  0 switches the guard off.
 *   "conv_i8_fold" (switch, default 1; SN_CONV_I8_NOFOLD=1 gives 0): 9 x 9 x 9 banks that are bit-for-bit symmetric in x and
 *       y (every GENEO bank) are contracted over 9 x 5 x 5 folded taps (exactly the same integer sums, a third of the
 *       MFMAs); the symmetry is checked on the device at every call, other banks take the unfolded kernel; 0 = never try
 *   "conv_i8_legacy" (switch, default 0; SN_CONV_I8_LEGACY=1 gives 1): 1 = sn_conv_bank uses the four-copy int8 kernel
 *       (conv_i8.hip) for every shape instead of the stride-4 kernel (conv_i8s.hip) it prefers for ky = 9 (A/B timing,
 *       parity tests of both).
 *   "conv_i8_no_stage" (switch, default 0; SN_CONV_I8_NO_STAGE=1 gives 1): 1 = the four-copy int8 kernel without its LDS-DMA
 *       staging.
 *   "conv_i8z_variant" (0 .. 2, default 2): the shape of the z-walk's tickets -- 0: rounds of two x-rows on 8 waves, 1: one
 *       round of one x-row per ticket on 12 waves, 2: two such rounds per ticket.  Same results bit for bit (tested on all
 *       three).
 *   "conv_no_i8" (switch, default 0; SN_CONV_NO_I8=1 gives 1): 1 = sn_conv_bank runs binary occupancy through the fp32
 *       kernel, never the int8 ones.
 *   "conv_double_buffer" (switch, default 0; SN_CONV_DOUBLE_BUFFER=1 gives 1): 1 = the fp32 kernel of sn_conv_bank on
 *       double-buffered 4 x 4 x 64 tiles instead of single-buffered 8 x 8 x 64 ones.
 *   "conv_lin_no24" (switch, default 0; SN_CONV_LIN_NO24=1 gives 1): 1 = sn_conv_fused packs its kernel rows in 32 bytes
 *       even where 24 would do.  Same results bit for bit.
 *   "voxel_onepass" (switch, default 1): sn_voxel_occupancy_fused[_bank] on grids whose bitmap(s) fit one workgroup's LDS
 *       (64^3) read the points ONCE -- bounding box, descriptor and binning in one launch whose workgroups exchange partial
 *       boxes; 0 = the two-kernel form (box pass, then binning pass).  Same results bit for bit.
 *   "voxel_onepass_spin" (>= 0, default 64): polls (~1 us each) a workgroup of that launch waits for its tile's other
 *       workgroups before it computes the tile's box from the points alone (same bits; 0 = never wait).
 *   "corr_dense" (switch, default 0; SN_CORR_DENSE=1 gives 1): 1 = the backward correlation of binary occupancy
 *       (sn_conv_corr*) as the GEMM form (K4) instead of the gather over the set voxels (K4s).
 *   "corr_sparse_tile_bytes" (0 .. 2048, default 0): input bytes per job of that gather (0: 2048, the maximum).
 *   "conv_i8z_inject_fault" (switch, default 0): TEST HOOK.  1 = the next z-walk launches never report plane 0's first raw
 *       rows as landed, so a dependency spin gives up (~0.5 s per launch): the way to see the loud failure path -- NaN
 *       outputs and the sticky device status -- on the product build (tests/test_gpu_conv_zwalk.py).
 *   "conv_i8z_segments" (0 .. 4, default 0): how the skipping z-walk cuts its columns in z.  1 = whole columns unless they do
 *       not fill the chip (the dense walk's plan); n >= 2 = n segments per column, segment sg of column xt dealt to the
 *       workgroup of column xt + sg max(1, nxt / n), where the shape allows it (a segment has at least 8 planes); on a head-only
 *       launch a workgroup then checks its own jobs, fills those whose operand region holds no set voxel without walking them
 *       and walks the rest.  0 = two such segments on head-only launches with Z >= 32 and at least two columns in x that the
 *       dense plan would walk as whole columns, else that plan.  Same results bit for bit; ignored under "conv_i8z_dense".
 *   "conv_i8z_trim" (switch, default 1): where the z-walk deals a tile's z segments by cost from the occupancy's row bits
 *       (sn_conv_bank_prepared_rows), a live segment streams only the range from its first to its last output plane whose
 *       operand window can hold a set voxel -- never fewer than min(8, segment) planes -- and the planes on either side are
 *       filled with the epilogue's constant.  Same results bit for bit; 0 = every live segment is streamed whole (the A/B
 *       switch).  No effect on any other launch.
 *   "conv_i8z_dense" (switch, default 0): the z-walk (sn_conv_bank_prepared[_served]) skips every round whose operand
 *       window -- 9 planes x 9 halo rows -- holds no set voxel and stores the epilogue's constant instead; the results are
 *       the same bit for bit (banks with a non-finite coefficient are never skipped), the run time depends on the data.
 *       1 = every round runs: the A/B switch, and the dense-convention figure benchmarks quote beside the default one. */
int sn_set_option(const char* name, int value);
int sn_get_option(const char* name);

/* ------------------------------------------------------------------------- *
 * K2  GENEO bank builder
 * replaces: GENEO_Layer.compute_kernel (core/models/SCENE_Net.py:103-106) over
 *           cylinderv2.compute_kernel (core/models/geneos/cylinder.py:162-176),
 *           arrow.compute_kernel      (core/models/geneos/arrow.py:228-252),
 *           negSpherev2.compute_kernel(core/models/geneos/neg_sphere.py:185-199),
 *           the v1 generators cylinder.py:84-103, arrow.py:173-205, neg_sphere.py:133-158,
 *           and the torch.stack at SCENE_Net.py:324 / :211.
 * params [G, SN_NPARAM] f32, kinds [G] i32 -> bank [G, kz, kx, ky] f32.
 * status (nullable) [G] i32: 0 ok, 1 = int(apex) outside [0, kz] (the reference
 * raises from torch.stack there; the kernel clamps and flags).
 * ------------------------------------------------------------------------- */
int sn_geneo_bank(const float* params, const int32_t* kinds, int G, int kz, int kx, int ky,
                  float* bank, int32_t* status, sn_stream_t stream);

/* The effective convex coefficients of SceneNet.forward (core/models/SCENE_Net.py:329-335):
 * out[g] = lambdas[g] except out[last] = (1 - sum_i lambdas[order[i]]) + lambdas[last], the sum taken sequentially in
 * fp32 in the order given (nn.ParameterDict order: names sorted) -- bit for bit what the reference's python `sum`
 * yields.  lambdas [G] f32 is in/out: lambdas[last] is overwritten with out[last], the side effect of
 * SCENE_Net.py:333 (the frozen parameter is refreshed by every forward).  order [G] i32, out [G] f32. */
int sn_effective_lambdas(float* lambdas, const int32_t* order, int G, int last, float* out, sn_stream_t stream);
/* sn_geneo_bank and sn_effective_lambdas in one launch (the two openers of a training forward: both read the packed
 * parameter vector, neither depends on the other). */
int sn_geneo_bank_lambdas(const float* params, const int32_t* kinds, int G, int kz, int kx, int ky, float* bank,
                          int32_t* status, float* lambdas, const int32_t* order, int last, float* lambdas_out,
                          sn_stream_t stream);
/* sn_geneo_bank_lambdas (lambdas nullable: then sn_geneo_bank) and sn_conv_bank_prep in ONE launch, for 9 x 9 x 9 kernels:
 * the workgroup that has just built kernel g prepares it for the int8 contraction from LDS (symmetry verdict, fixed-point
 * weights, error bound, digit-table entries; see sn_conv_bank_prep below).  prep: SN_CONV_PREP_BYTES x ceil(G / 16),
 * 16-byte aligned.  Neither the bank nor the blob depends on the voxel grid: the launch can run on a side stream next to
 * the voxelisation and be joined in front of sn_conv_bank_prepared. */
int sn_geneo_bank_prep(const float* params, const int32_t* kinds, int G, int kz, int kx, int ky, float* bank,
                       int32_t* status, float* lambdas, const int32_t* order, int last, float* lambdas_out,
                       void* prep, sn_stream_t stream);

/* ------------------------------------------------------------------------- *
 * K3  GENEO bank convolution + convex-combination head
 * replaces: SceneNet.forward (core/models/SCENE_Net.py:322-339):
 *           F.conv3d(x, kernels, padding='same') (cross-correlation, zero pad
 *           left (k-1)/2, right k/2), sum_i lambda_i * conv_i, relu(tanh(.)).
 * x [B,1,Z,X,Y] of x_dtype; bank [G,kz,kx,ky] f32; lambdas [G] f32 = the
 * EFFECTIVE coefficients (last one already 1 - sum(others)), nullable iff out
 * is null.  act (nullable) [B,G,Z,X,Y] and out (nullable) [B,1,Z,X,Y] are of
 * out_dtype (SN_F32 or SN_F64).  x_dtype SN_F32 / SN_F64 / SN_U8: fp32 MFMA accumulation
 * (v_mfma_f32_16x16x4_f32).  x_dtype SN_OCC8 (values in {0,1}): weights as 24-bit fixed point in three
 * int8 digits, exact int32 accumulation on v_mfma_i32_16x16x64_i8, recombined in fp32.
 * Any G: one MFMA row block holds 16 kernels, larger banks run as ceil(G/16) launches with the raw partial sum
 * carried in `out` (the last launch applies relu(tanh)).
 * ------------------------------------------------------------------------- */
int sn_conv_bank(const void* x, int x_dtype, const float* bank, const float* lambdas,
                 int B, int Z, int X, int Y, int G, int kz, int kx, int ky,
                 void* act, void* out, int out_dtype, sn_stream_t stream);

/* What sn_conv_bank would launch for these arguments under the options in force now: host arithmetic only, no launch, no
 * device memory; works without a device (the tile ladder then assumes 256 compute units).  It runs the planners the launch
 * itself runs, so the two cannot disagree; pointers are taken to be aligned the way a fresh allocation is (16 bytes).  For
 * G > 16 it describes the launch of the first group of 16 kernels.  plan8 (8 x int32, host memory):
 *   [0] kernel: 0 the fp32 MFMA kernel, 1 the four-copy int8 kernel, 2 the stride-4 int8 kernel, 3 the folded int8 kernel
 *       (the host's half of that choice: the launch is the folded kernel's, which checks the bank's x/y symmetry on the
 *       device and runs the stride-4 body in place, on the same tiles, for a bank that is not symmetric).  The guards that
 *       hand an int8 launch to the fp32 kernel on the device (conv_i8_tolerance_ppb) are not part of the plan
 *   [1] TZ, [2] TX: z and x extent of a workgroup tile (its y extent is always 64)
 *   [3] number of workgroup tiles: B * ceil(Z / TZ) * ceil(X / TX) * ceil(Y / 64)
 *   [4] flags: bit 0 the fp32 kernel's double-buffered form, bit 1 the halo is staged by LDS-DMA
 *   [5] stride of a halo row in LDS, bytes
 *   [6] compute units the tile ladder counted (the first rung with [3] >= 4 * [6] is taken)
 *   [7] 0 (reserved)
 * Returns SN_OK, SN_ERR_INVALID_ARG (null plan8, an extent <= 0, unknown x_dtype) or SN_ERR_UNSUPPORTED where sn_conv_bank
 * returns it (ky > 25, kernel does not fit LDS).  No reference counterpart (F.conv3d has no tile plan to ask about): this is
 * what lets a test reach, and name, every tile the hand-written kernels can pick. */
int sn_conv_bank_plan(int x_dtype, int B, int Z, int X, int Y, int G, int kz, int kx, int ky, int32_t* plan8);

/* The same contraction for a bank whose per-bank work was done once, ahead of the launch (round 3).
 * SceneNet.forward rebuilds its kernels from the parameters on every call (SCENE_Net.py:322-327); everything the int8
 * contraction derives from the bank alone -- the x/y symmetry verdict, the 24-bit fixed-point weights, the worst-case
 * quantisation error per kernel, the digit table of the folded operand plan -- is a function of those weights, so
 * sn_conv_bank_prep computes it in one small launch (16 workgroups; it can run on a side stream next to the
 * voxelisation) into `prep`: caller-owned device memory, 16-byte aligned, SN_CONV_PREP_BYTES per group of 16 kernels
 * (ceil(G / 16) groups).  sn_conv_bank_prepared is sn_conv_bank with that blob: SN_OCC8 input and a 9 x 9 x 9 bank run
 * the z-walk kernel (csrc/conv_i8z.inc: every input plane fetched and y-folded once per 8 x 64 column, no per-workgroup
 * prologue); the blob also holds the launch's route flag (bank not symmetric: the unfolded body runs in the same
 * launch; quantisation bound over the tolerance: the gated fp32 launch behind it takes over), so a captured graph owns
 * its flag.  One blob serves the launches of ONE stream at a time.  Results are bit-identical to sn_conv_bank's.
 * Every other dtype / shape: forwarded to sn_conv_bank (prep may be null). */
#define SN_CONV_PREP_BYTES 16384
int sn_conv_bank_prep(const float* bank, int G, int kz, int kx, int ky, void* prep, sn_stream_t stream);
int sn_conv_bank_prepared(const void* x, int x_dtype, const float* bank, const float* lambdas, void* prep,
                          int B, int Z, int X, int Y, int G, int kz, int kx, int ky,
                          void* act, void* out, int out_dtype, sn_stream_t stream);
/* sn_conv_bank_prepared without the fallback launch behind the walk.  The walk's verdict -- 0 served, 1 quantisation bound
 * over the tolerance (fp32 form), 2 bank not symmetric (unfolded body) -- is an int32 at byte offset
 * sn_conv_prep_verdict_offset() of each group's blob, written by every walk launch; it depends on the weights, the
 * coefficients, the tolerance and on which outputs are asked for, on nothing else.  A caller that has READ it as 0 for
 * exactly these (e.g. a serving loop whose parameters do not change: read it back once, asynchronously) may use this entry:
 * the ~3 us empty dispatch of the fallback launch disappears.  If the verdict is NOT 0 -- the caller's knowledge was stale --
 * the launch fills `out` / `act` with NaN and latches the sticky device status (code 2, sn_device_status): the call itself
 * has returned SN_OK by then (it is asynchronous), the NEXT sn_* call on the device fails with SN_ERR_DEVICE_STATUS.  It
 * never leaves the outputs unwritten. */
int sn_conv_bank_prepared_served(const void* x, int x_dtype, const float* bank, const float* lambdas, void* prep,
                                 int B, int Z, int X, int Y, int G, int kz, int kx, int ky,
                                 void* act, void* out, int out_dtype, sn_stream_t stream);
/* sn_conv_bank_prepared (assume_served = 0) / _served (1) with the occupancy's ROW BITS: rows[b][z][w] uint32, w < ceil(X / 32),
 * bit x % 32 of word x / 32 set iff x[b, 0, z, x, :] holds a set voxel (a SUPERSET is allowed and costs time only; a missing
 * bit is a wrong result: hand in only bits that describe x as it is now).  sn_voxel_occupancy_fused_rows writes them.  rows =
 * NULL: exactly the two entries above.  With bits, the head-only z-walk of a grid with Y <= 64, Z <= 64, X <= 64 whose launch
 * has one workgroup per 8-row column (B ceil(X / 8) = the device's compute units) cuts the columns into four z segments where
 * Z = 64 (option "conv_i8z_segments" = 0; else the count it names, which must divide Z) and deals each tile's segments over
 * that tile's workgroups by cost (csrc/conv_i8z.inc, THE BALANCED DEAL): same results bit for bit.  Any other launch --
 * another batch size, 128^3, the activations form -- takes the plan it takes without bits, segment count included, and does
 * not read them: the gain is confined to one batch size per grid and device.
 * plan_out (nullable, diagnostics; the caller sizes it by the device's compute units): int32 [compute units][65], row w = (n, the n job numbers of workgroup w in its order;
 * job number = segment x B ceil(X / 8) + tile x ceil(X / 8) + column slot), written only where the balanced deal runs. */
int sn_conv_bank_prepared_rows(const void* x, int x_dtype, const float* bank, const float* lambdas, void* prep,
                               int B, int Z, int X, int Y, int G, int kz, int kx, int ky,
                               void* act, void* out, int out_dtype, sn_stream_t stream, int assume_served,
                               const uint32_t* rows, int32_t* plan_out);
int sn_conv_prep_verdict_offset(void);
/* Diagnostics: how many waves of the int8 kernels ever gave up a bounded LDS hand-over spin (must stay 0).  A give-up is
 * not silent: it latches the sticky device status (code 1 / 3, above), and the z-walk overwrites its workgroup's outputs
 * with NaN.  Synchronises the device. */
int sn_conv_i8_spin_timeouts(unsigned long long* count);
/* Diagnostics: rounds the z-walk ran [0] and skipped because their operand window was empty [1] (see "conv_i8z_dense"), all
 * launches of this process on the device.  Each workgroup adds its sums once, at its end.  Synchronises the device. */
int sn_conv_i8z_round_counts(unsigned long long* counts2);
/* ... input planes the head-only z-walk streamed [0] and planes it did not stream because "conv_i8z_trim" cut them from a
 * live segment [1], all launches since the library was loaded.  [0] counts EVERY head-only launch of the walk -- dense,
 * static and dealt plans alike, whether or not anything can be trimmed; a z segment that is filled without being walked
 * streams nothing and adds nothing.  Launches that write the per-kernel activations are not counted.  Synchronises. */
int sn_conv_i8z_plane_counts(unsigned long long* counts2);
/* Diagnostics: how many workgroups of the one-pass voxelisation kernel (sn_voxel_occupancy_fused[_bank] at grids whose bitmap
 * fits one workgroup) ever gave up the bounded wait of the box exchange and took their tile's box from the points themselves
 * -- the same bits, one more pass over the tile.  0 in normal use; every workgroup with option voxel_onepass_spin = 0.
 * Counted by the kernel itself (no launch of its own), in a word of the CURRENT device: the count is per device and per
 * process, cumulative from the library's load -- there is no reset, compare two readings.  Synchronises the device. */
int sn_voxel_onepass_giveups(unsigned long long* count);

/* Measurement hook: the NEXT z-walk launch of the calling thread (sn_conv_bank_prepared[_served] on a 9^3 bank) is made with
 * hipExtLaunchKernel(..., start_event, stop_event): the two hipEvent_t (created by the caller; either may be null) receive
 * the kernel's own start and stop timestamps -- what a profiler's kernel trace reports -- instead of the interval between two
 * hipEventRecord around the call, which includes the records' own ~2.5 us on the stream and the launch's dispatch.  One-shot:
 * consumed by that launch (or by a later one if this one takes another kernel).  bench.py times the dominant kernel with it.
 * The reference has no counterpart (its profiler is torch.profiler around core/models/SCENE_Net.py:322-339). */
int sn_launch_timing_events(void* start_event, void* stop_event);

/* The same forward output through linearity, without materialising the bank activations:
 *   relu(tanh(sum_g lambda_g conv3d(x, K_g))) == relu(tanh(conv3d(x, sum_g lambda_g K_g)))
 * (equal to 5e-16 in the reference's fp64; core/models/SCENE_Net.py:322-339).  One combined kernel
 * K* = sum_g lambda_g K_g (any G), 24-bit fixed point, Toeplitz-along-y implicit GEMM on v_mfma_i32_16x16x64_i8:
 * 0.375 MFMA per voxel at 9^3 (kernel rows packed at 24 K-bytes for ky <= 9; 0.48 otherwise) instead of 3.  x: SN_OCC8 only ([B,1,Z,X,Y], values in {0,1}, Y % 4 == 0, ky <= 17);
 * out [B,1,Z,X,Y] SN_F32 | SN_F64 | SN_BF16.  Returns SN_ERR_UNSUPPORTED for other inputs / shapes: call sn_conv_bank then.
 * Error vs the 16-kernel contraction: the fixed-point step of K* (<= 2^-23 max|K*| per tap) and fp32 rounding of
 * the combination, ~1e-6 on the output. */
int sn_conv_fused(const void* x, int x_dtype, const float* bank, const float* lambdas, int B, int Z, int X, int Y,
                  int G, int kz, int kx, int ky, void* out, int out_dtype, sn_stream_t stream);
/* sn_conv_fused with the guard's verdict in a caller-owned device word (0: served by the combined int8 kernel, 1: its
 * quantisation bound exceeded the tolerance and the gated fp32 launches behind took over) -- the verdict depends on the
 * weights, the coefficients and the tolerance only, so a caller that has READ 0 for these very parameters may pass
 * assume_served = 1 and the (then empty) gated launches are left out, as sn_conv_bank_prepared_served does for the
 * contraction.  bf16 output runs unguarded (the verdict is then not written). */
int sn_conv_fused_v(const void* x, int x_dtype, const float* bank, const float* lambdas, int B, int Z, int X, int Y, int G,
                    int kz, int kx, int ky, void* out, int out_dtype, int32_t* verdict, int assume_served,
                    sn_stream_t stream);
/* The per-(bank, coefficients) work of sn_conv_fused -- K* = sum_g lambda_g K_g, its 24-bit fixed point, the worst-case
 * error bound and the Toeplitz digit tables: ~8 us that every workgroup of the kernel otherwise spends for itself -- once,
 * into a caller-owned blob of sn_conv_fused_prep_bytes(kz, kx, ky) bytes (16-byte aligned; 0: kernel extent not served),
 * and the forward on that blob: same results bit for bit.  The blob carries the guard's verdict at the tolerance in force
 * when it was written (sn_conv_fused_v's word: byte offset bytes - 12); assume_served as there. */
size_t sn_conv_fused_prep_bytes(int kz, int kx, int ky);
int sn_conv_fused_prep(const float* bank, const float* lambdas, int G, int kz, int kx, int ky, void* blob,
                       sn_stream_t stream);
int sn_conv_fused_prepared(const void* x, int x_dtype, const float* bank, const float* lambdas, const void* blob, int B,
                           int Z, int X, int Y, int G, int kz, int kx, int ky, void* out, int out_dtype, int assume_served,
                           sn_stream_t stream);


/* 1 when sn_conv_fused serves a [B,1,Z,X,Y] SN_OCC8 grid with a [kz,kx,ky] kernel (Y % 4, the ky window, the tables and
 * the halo within 160 KiB of LDS), else 0: the caller's dispatch predicate, from the same plan the launch uses. */
int sn_conv_fused_supported(int B, int Z, int X, int Y, int kz, int kx, int ky);

/* What sn_conv_fused (and its _v / _prepared forms) would launch for these arguments under the options in force now: host
 * arithmetic only, no launch, no device memory; works without a device (256 compute units are then counted).  The shape
 * plan is the launch's own (the one sn_conv_fused_supported answers from), and the grid size and the deferral rule come
 * from the helper the launch and the kernel themselves call, so the query cannot drift from them.  The kernel is
 * persistent: workgroup w walks tiles w, w + [5], w + 2 [5], ...; the next tile's halo is requested into registers while the
 * current tile's MFMAs run, and with a deferred epilogue a tile's outputs are activated and stored between the MFMAs of the
 * workgroup's NEXT tile -- both only from a workgroup's second tile on, i.e. where [4] > [5].  plan8 (8 x int32, host memory):
 *   [0] 1: kernel rows packed at 24 bytes of K (ky <= 9 and option "conv_lin_no24" = 0), 0: at 32 bytes
 *   [1] MFMA steps per tile: ceil(3 kz kx / 8) at 24 bytes, ceil(kz kx / 2) at 32
 *   [2] 1: deferred epilogue ([1] >= 16), 0: every tile is finished at once
 *   [3] halo passes per tile, ceil(halo rows / 25) with (8 + kz - 1)(16 + kx - 1) halo rows: the first 16 passes travel
 *       through registers, more than 16 means the synchronous remainder pass runs
 *   [4] workgroup tiles (8 x 16 x 64): B * ceil(Z / 8) * ceil(X / 16) * ceil(Y / 64)
 *   [5] workgroups launched: min([7], [4])
 *   [6] dynamic LDS of the launch, bytes
 *   [7] compute units counted
 * G enters the kernel's prologue only (any G > 0 gives the same plan).  Returns SN_OK, SN_ERR_INVALID_ARG (null plan8, an
 * extent <= 0) or SN_ERR_UNSUPPORTED where sn_conv_fused returns it (Y % 4 != 0, ky window, LDS).  No reference counterpart
 * (F.conv3d has no tile walk to ask about): this is what lets tests/test_gpu_conv_lin_walk.py size a batch so that every
 * workgroup walks several tiles on the device at hand, and name the fork of the kernel a case ran. */
int sn_conv_fused_plan(int B, int Z, int X, int Y, int G, int kz, int kx, int ky, int32_t* plan8);

/* SceneNet.forward for FLOAT grids that are usually binary occupancy -- what the reference itself feeds: f64 {0., 1.}
 * out of ToFullDense (core/datasets/torch_transforms.py:33-34).  One pass writes (x != 0) into occ_ws [B*Z*X*Y] bytes
 * and raises not_binary[0] when an element is neither 0 nor 1; then the int8 form (sn_conv_fused on the bytes, or
 * sn_conv_bank where that does not serve the shape) and the fp32 form (sn_conv_bank on x) of the same forward are
 * BOTH enqueued, each gated on that device flag: one runs, the other exits in its first instruction.  No host
 * synchronisation, same output contract as sn_conv_bank(out only).  x: SN_F32 | SN_F64, 16-byte aligned; occ_ws 4-byte
 * aligned; out: SN_F32 | SN_F64.  Every argument is checked before the first launch: SN_ERR_INVALID_ARG (a null pointer, an
 * extent <= 0, another x_dtype or out_dtype, a misaligned x or occ_ws; sn_last_error() names the argument) and
 * SN_ERR_UNSUPPORTED (a shape sn_conv_bank_plan refuses) leave occ_ws, not_binary and out untouched. */
int sn_forward_auto(const void* x, int x_dtype, const float* bank, const float* lambdas, int B, int Z, int X, int Y,
                    int G, int kz, int kx, int ky, uint8_t* occ_ws, int32_t* not_binary, void* out, int out_dtype,
                    sn_stream_t stream);

/* ------------------------------------------------------------------------- *
 * K1  point cloud -> voxel grid
 * replaces: pyntcloud VoxelGrid.compute as called by eda.voxelize_ply
 *           (utils/pcd_processing.py:341-372), hist_on_voxel
 *           (utils/voxelization.py:164-204), reg_on_voxel (:244-300),
 *           normalize_xyz (utils/pcd_processing.py:305-321) and
 *           ToFullDense.densify (core/datasets/torch_transforms.py:33-34).
 *
 * A batch is ragged: pts [total,3] f64 (x,y,z), labels [total] f64 (nullable),
 * offsets [B+1] i64 (CSR: tile b owns points offsets[b] .. offsets[b+1]-1).
 * ------------------------------------------------------------------------- */

/* doubles per tile in a grid descriptor: lo[3], hi[3], then the linspace edge
 * tables of x (nx+1), y (ny+1), z (nz+1). */
#define SN_DESC_LEN(nx, ny, nz) (6 + (nx) + (ny) + (nz) + 3)

/* Per-tile bounding box: bbox [B,6] f64 = (min x,y,z, max x,y,z). */
int sn_voxel_bbox(const double* pts, const int64_t* offsets, int B, double* bbox, sn_stream_t stream);

/* sn_voxel_bbox + sn_voxel_desc in two launches (no atomics, nothing to initialise) for the batch pipeline:
 * partial_ws is scratch [B, SN_BBOX_PARTS, 6] f64; bbox (nullable) receives the raw boxes. */
#define SN_BBOX_PARTS 32
int sn_voxel_prepare(const double* pts, const int64_t* offsets, int B, int nx, int ny, int nz, int regular,
                     double* partial_ws, double* bbox, double* desc, sn_stream_t stream);

/* Grid descriptor from a bounding box, n_x/n_y/n_z mode
 * (add_structure("voxelgrid", n_x, n_y, n_z), pcd_processing.py:362-363):
 * regular != 0 pads the box to a cube (pyntcloud regular_bounding_box=True);
 * edges are numpy.linspace(lo, hi, n+1) bit for bit.  desc [B, SN_DESC_LEN]. */
int sn_voxel_desc(const double* bbox, int B, int nx, int ny, int nz, int regular,
                  double* desc, sn_stream_t stream);

/* Same, from explicit per-tile bounds [B,6] (lo xyz, hi xyz) the caller has
 * already extended -- used for the size_x/size_y/size_z mode
 * (pcd_processing.py:365-367), whose grid extents are data dependent. */
int sn_voxel_desc_from_bounds(const double* bounds, int B, int nx, int ny, int nz,
                              double* desc, sn_stream_t stream);

/* Grid descriptor in the size_x/size_y/size_z mode for a whole batch, computed on the device
 * (replaces: pyntcloud VoxelGrid.compute with sizes, utils/pcd_processing.py:365-367, as used by
 * core/datasets/semKITTI.py:453-455): cube the box, extend every axis by ((range // size) + 1) * size - range, n =
 * int((max - min) / size) -- numpy's fp64 arithmetic bit for bit.  n is data dependent, so grids are allocated at a
 * caller-given maximum (nx, ny, nz) and desc [B, SN_DESC_LEN(nx,ny,nz)] carries each tile's own edge tables: edges
 * 0..n_a as numpy.linspace, +inf beyond.  sn_voxel_scatter / sn_gather_points take this descriptor unchanged;
 * sn_voxel_finalize_sized keeps the voxels beyond a tile's own dims out of the column statistics and zero.
 *   size_xyz_host  3 doubles on the host (voxel size per axis, > 0)
 *   dims           (nullable) [B,3] i32 out: n_x, n_y, n_z of every tile
 *   status         (nullable) [B] i32 out: 1 = the tile needs more voxels than the maximum (points beyond the table
 *                  are dropped and counted by the scatter)
 * For the scatter and the LDS-bitmap kernels a size-mode descriptor is defined only for the points it was built from
 * (none of them is above its tile's own last edge).  They bin with the padded table as it stands: a foreign point above
 * a tile's own last edge on an axis with n_a < the maximum lands in the padding cell n_a of that axis, is counted there
 * and is NOT reported in `dropped`.  sn_gather_points alone treats such a point as outside (`fill`). */
int sn_voxel_desc_sized(const double* bbox, int B, const double* size_xyz_host, int nx, int ny, int nz,
                        double* desc, int32_t* dims, int32_t* status, sn_stream_t stream);

/* sn_voxel_finalize for grids voxelised with a size-mode descriptor (normalize_xyz / ToFullDense over each tile's
 * own [n_z, n_x, n_y] part of the padded grid; the rest is 0). */
int sn_voxel_finalize_sized(const int32_t* counts, const int32_t* tower_counts, int B, int nx, int ny, int nz,
                            const double* desc, int32_t* colstats, double* density, double* gt, float* occ,
                            float* gt_occ, sn_stream_t stream);

/* Atomic scatter: counts[b,z,x,y] += 1 per point; tower_counts (nullable) += 1
 * per point whose label equals one of keep_labels_host[0..n_keep) (<= 16).
 * Both grids [B,nz,nx,ny] i32 are zeroed by the call.
 * The binning rule, for ANY point (the descriptor need not come from these points -- a fixed box, a crop's grid): per
 * axis the index is np.clip(np.searchsorted(edges, p, side="left") - 1, 0, n), i.e. the largest j with edges[j] < p.  A
 * point at or below the first edge (-inf included) is clipped into bin 0 and counted there; index n on any axis -- a
 * point above the last edge, +inf -- or a NaN coordinate means outside the table: the point is counted in no voxel.
 * dropped (nullable) [B] i32: the points outside the edge table, each once; counts.sum() + dropped == the tile's points. */
int sn_voxel_scatter(const double* pts, const double* labels, const int64_t* offsets, int B,
                     const double* desc, int nx, int ny, int nz,
                     int32_t* counts, int32_t* tower_counts,
                     const double* keep_labels_host, int n_keep,
                     int32_t* dropped, sn_stream_t stream);

/* counts -> outputs (each nullable):
 *   density [B,1,nz,nx,ny] f64 : hist_on_voxel's per-y-column min-max normalised counts
 *   gt      [B,1,nz,nx,ny] f64 : reg_on_voxel's tower/total ratio (needs tower_counts)
 *   occ     [B,1,nz,nx,ny] f32 : ToFullDense(density)  == (density > 0)
 *   gt_occ  [B,1,nz,nx,ny] f32 : ToFullDense(gt)       == (tower > 0)
 * colstats: workspace [B, 2, ny] i32. */
int sn_voxel_finalize(const int32_t* counts, const int32_t* tower_counts, int B, int nx, int ny, int nz,
                      int32_t* colstats, double* density, double* gt, float* occ, float* gt_occ,
                      sn_stream_t stream);

/* Occupancy-only form of the same step, for the fused pipeline: what SceneNet consumes is
 * ToFullDense(Voxelization(points)) (scripts/main.py:138-140), one bit per voxel.  Workgroups build the tile's
 * bitmap in LDS (no global atomics) and the result is expanded to occ / gt_occ [B,1,nz,nx,ny] of out_dtype
 * (SN_U8 or SN_F32); gt_occ nullable.  Needs nx*ny*nz % 32 == 0 and the bitmap(s) of one of <= SN_OCC_PARTS
 * z-slabs to fit 64 KiB of LDS (64^3: one slab; 128^3: 4 slabs, 8 with gt_occ); otherwise SN_ERR_UNSUPPORTED ->
 * use sn_voxel_scatter + sn_voxel_finalize.
 *   bits_ws     scratch, SN_OCC_WS_WORDS(B, nx*ny*nz, planes) uint32 (planes = 2 with gt_occ, else 1)
 *   flags       (nullable) [B] i32 out: 1 = the tile could not be proven free of a fully occupied y column
 *               (where ToFullDense(density) != (count > 0)); such tiles are recomputed exactly (counts by
 *               global atomics, column minima) by one gated launch when counts_ws (and towers_ws with
 *               gt_occ) is given: counts_ws, towers_ws [B,nz,nx,ny] i32 scratch (nullable).
 *   dropped     (nullable) [B] i32: points outside the edge table, each once however many z-slabs the bitmap takes.
 * Binning rule as sn_voxel_scatter's, for any point: below the first edge -> bin 0; above the last edge, +inf or NaN ->
 * outside (sets no bit, counted in dropped) -- in the bitmap kernels and in the exact recomputation alike. */
#define SN_OCC_PARTS 16
#define SN_OCC_WS_WORDS(B, V, planes) ((size_t)(B) * SN_OCC_PARTS * ((planes) * ((V) / 32) + 1))
int sn_voxel_occupancy(const double* pts, const double* labels, const int64_t* offsets, int B,
                       const double* desc, int nx, int ny, int nz,
                       const double* keep_labels_host, int n_keep,
                       uint32_t* bits_ws, void* occ, void* gt_occ, int out_dtype,
                       int32_t* flags, int32_t* dropped,
                       int32_t* counts_ws, int32_t* towers_ws, sn_stream_t stream);

/* sn_voxel_prepare + sn_voxel_occupancy in four launches instead of five: the binning kernel derives the tile's
 * descriptor (cube regularisation, numpy.linspace edges: the same instruction sequence, the same bits) from the bbox
 * partials itself and publishes it in `desc` [B, SN_DESC_LEN] (and the raw box in `bbox` [B,6], nullable) for the later
 * kernels and callers.  partial_ws: scratch [B, SN_BBOX_PARTS, 6] f64.  Everything else as sn_voxel_occupancy. */
int sn_voxel_occupancy_fused(const double* pts, const double* labels, const int64_t* offsets, int B, int nx, int ny,
                             int nz, int regular, const double* keep_labels_host, int n_keep, double* partial_ws,
                             double* bbox, double* desc, uint32_t* bits_ws, void* occ, void* gt_occ, int out_dtype,
                             int32_t* flags, int32_t* dropped, int32_t* counts_ws, int32_t* towers_ws,
                             sn_stream_t stream);
/* ... which also writes the occupancy's row bits (layout: sn_conv_bank_prepared_rows) into row_bits [B][nz][ceil(nx / 32)]
 * (nullable).  A tile whose flag goes up is rewritten by the exact fallback to a subset of what the bits describe: its bits
 * stay a superset. */
int sn_voxel_occupancy_fused_rows(const double* pts, const double* labels, const int64_t* offsets, int B, int nx, int ny,
                                  int nz, int regular, const double* keep_labels_host, int n_keep, double* partial_ws,
                                  double* bbox, double* desc, uint32_t* bits_ws, void* occ, void* gt_occ, int out_dtype,
                                  int32_t* flags, int32_t* dropped, int32_t* counts_ws, int32_t* towers_ws,
                                  sn_stream_t stream, uint32_t* row_bits);

/* What sn_voxel_occupancy (fused = 0: a descriptor is given), sn_voxel_occupancy_fused (fused = 1: the tile's own box) or
 * sn_voxel_occupancy_sized (sized = 1) would launch for an (nx, ny, nz) grid with `planes` bitmaps (2 with gt_occ, else 1)
 * and B tiles under the options in force now: host arithmetic only, no launch, no device memory, works without a device.
 * It evaluates the very text the launches and occ_finalize_kernel evaluate, so they cannot disagree.  The alignment arguments (0 / 1)
 * say whether pts, labels and bits_ws are 16-byte aligned; want_flags whether `flags` is given.  plan8 (8 x int32, host):
 *   [0] 1: the one-pass kernel (box, descriptor and bitmap in one launch), 0: the two-kernel form
 *   [1] z-slabs of the LDS bitmap (1, 2, 4, 8 or 16)
 *   [2] partial bitmaps per tile that the finalize kernel ORs
 *   [3] the emptiness proof: 0 none (no flags), 1 on the merged words of the expansion loop, 2 a second pass over the rows
 *   [4] 1: the finalize kernel takes four words per thread, 0: one
 *   [5] ny / 32: whole words per (z, x) row
 *   [6] workgroups per tile of the finalize launch
 *   [7] dynamic LDS of the binning launch, bytes
 * Returns SN_OK, SN_ERR_INVALID_ARG (null plan8, an extent or B <= 0, planes outside 1..2) or SN_ERR_UNSUPPORTED exactly
 * where the launch returns it (no z-slab count fits).  No reference counterpart: this is what lets a test reach, and name,
 * every fork of the bitmap kernels. */
int sn_voxel_occupancy_plan(int nx, int ny, int nz, int planes, int B, int fused, int sized, int pts_aligned16,
                            int labels_aligned16, int ws_aligned16, int want_flags, int32_t* plan8);

/* sn_voxel_occupancy_fused with K2 riding in its first launch: the workgroups that build the 9 x 9 x 9 GENEO bank and the
 * int8 contraction's preparation blob (exactly sn_geneo_bank_prep's: the same arguments from `params` to `prep`, the same
 * bits; with `lambdas` the effective coefficients ride too, as in a training forward's opener sn_geneo_bank_lambdas) are extra grid rows of the bounding-box kernel, so the inference step has no launch, no stream fork and no
 * event for K2 at all ([measured] the forked form left 10.8 of K2's 12.4 serial microseconds on the critical path).
 * Replaces, for the hot path, GENEO_Layer.compute_kernel x G (SCENE_Net.py:103-106, 322-324) next to
 * Voxelization.__call__ (torch_transforms.py:74-81). */
int sn_voxel_occupancy_fused_bank(const double* pts, const double* labels, const int64_t* offsets, int B, int nx, int ny,
                                  int nz, int regular, const double* keep_labels_host, int n_keep, double* partial_ws,
                                  double* bbox, double* desc, uint32_t* bits_ws, void* occ, void* gt_occ, int out_dtype,
                                  int32_t* flags, int32_t* dropped, int32_t* counts_ws, int32_t* towers_ws,
                                  const float* params, const int32_t* kinds, int G, int kz, int kx, int ky, float* bank,
                                  int32_t* status, float* lambdas, const int32_t* order, int last, float* lambdas_out,
                                  void* prep, sn_stream_t stream);
int sn_voxel_occupancy_fused_bank_rows(const double* pts, const double* labels, const int64_t* offsets, int B, int nx, int ny,
                                       int nz, int regular, const double* keep_labels_host, int n_keep, double* partial_ws,
                                       double* bbox, double* desc, uint32_t* bits_ws, void* occ, void* gt_occ, int out_dtype,
                                       int32_t* flags, int32_t* dropped, int32_t* counts_ws, int32_t* towers_ws,
                                       const float* params, const int32_t* kinds, int G, int kz, int kx, int ky, float* bank,
                                       int32_t* status, float* lambdas, const int32_t* order, int last, float* lambdas_out,
                                       void* prep, sn_stream_t stream, uint32_t* row_bits);

/* sn_voxel_occupancy_fused in VOXEL-SIZE mode (voxelize_ply with size_x / size_y / size_z, utils/pcd_processing.py:365-367;
 * the mode SemanticKITTI uses, core/datasets/semKITTI.py:453-455): every tile's grid extents follow from its own bounding
 * box -- computed on the device as in sn_voxel_desc_sized, no host round trip -- and the binary grids are written padded
 * to the maximum (nx, ny, nz): dims [B,3] i32 = each tile's own (n_x, n_y, n_z), status [B] i32 (nullable) = 1 where a
 * tile needs more than the maximum (its points beyond are dropped), voxels beyond a tile's own dims are 0.  Same
 * LDS-bitmap kernels (no global atomic per point), same workspaces and outputs as sn_voxel_occupancy_fused; the
 * "count > column minimum" rule of ToFullDense(normalize_xyz(.)) is evaluated over each tile's OWN part of the grid. */
int sn_voxel_occupancy_sized(const double* pts, const double* labels, const int64_t* offsets, int B,
                             const double* size_xyz_host, int nx, int ny, int nz,
                             const double* keep_labels_host, int n_keep, double* partial_ws, double* bbox,
                             double* desc, int32_t* dims, int32_t* status, uint32_t* bits_ws, void* occ,
                             void* gt_occ, int out_dtype, int32_t* flags, int32_t* dropped,
                             int32_t* counts_ws, int32_t* towers_ws, sn_stream_t stream);
/* sn_voxel_occupancy_sized with the same riders as sn_voxel_occupancy_fused_bank (C4's chain: voxel-size mode -> conv). */
int sn_voxel_occupancy_sized_bank(const double* pts, const double* labels, const int64_t* offsets, int B,
                                  const double* size_xyz_host, int nx, int ny, int nz, const double* keep_labels_host,
                                  int n_keep, double* partial_ws, double* bbox, double* desc, int32_t* dims, int32_t* status,
                                  uint32_t* bits_ws, void* occ, void* gt_occ, int out_dtype, int32_t* flags,
                                  int32_t* dropped, int32_t* counts_ws, int32_t* towers_ws, const float* params,
                                  const int32_t* kinds, int G, int kz, int kx, int ky, float* bank, int32_t* bank_status,
                                  float* lambdas, const int32_t* order, int last, float* lambdas_out, void* prep,
                                  sn_stream_t stream);


/* Grid -> points: out[c, i] = grid[b(i), c, vz, vx, vy] for every point i of the batch, binned exactly as the
 * scatter binned it (same desc); points outside the edge table get `fill`.  The points need not be the ones the
 * descriptor was built from (labelling a full cloud from the grid of a crop): the rule is sn_voxel_scatter's -- at or
 * below the first edge of an axis (-inf included) -> bin 0; above the last edge, +inf or NaN -> outside -> `fill` (any
 * value, NaN included).  With a size-mode descriptor the last edge is the tile's OWN (edge n_a, the last finite one):
 * the +inf padding beyond it is not part of the tile's grid.  grid [B,channels,nz,nx,ny] and out [channels, total] are
 * of `dtype` (SN_F32 | SN_F64); total = offsets[B] is the channel stride of `out`, so `pts` holds exactly that many
 * points as far as `out` is concerned; desc is [B, SN_DESC_LEN(nx,ny,nz)].  The reference only has the voxel-list direction
 * (vxg_to_xyz, utils/voxelization.py:328-360) and prob_to_label (:304-323); per-point read-back of the
 * prediction (BASELINE config 4) is defined here. */
int sn_gather_points(const void* grid, int dtype, int channels, const double* pts, const int64_t* offsets, int B,
                     const double* desc, int nx, int ny, int nz, double fill, void* out, sn_stream_t stream);

/* Grid -> voxel list (vxg_to_xyz, utils/voxelization.py:328-360): EVERY cell of the [n0,n1,n2] grid, in C order
 * of its indices (np.indices(shape).reshape(3,-1).T), as a row  out[n] = (origin + index * voxel_size, grid[index]),
 * fp64 like the reference's np.concatenate result.  origin / voxel_size: 3 host doubles each, null = (0,0,0) /
 * (1,1,1) (the reference defaults).  grid of `dtype` (SN_F32 | SN_F64 | SN_U8 | SN_OCC8); out [n0*n1*n2, 4] f64,
 * 16-byte aligned.  The product is formed and then added (two roundings, as numpy does). */
int sn_grid_to_points(const void* grid, int dtype, int n0, int n1, int n2, const double* origin_host,
                      const double* voxel_size_host, double* out, sn_stream_t stream);

/* ------------------------------------------------------------------------- *
 * Backward (training config; reference: autograd through SceneNet.forward, SCENE_Net.py:322-339, and the
 * generator graphs cylinder.py / arrow.py / neg_sphere.py).  By linearity the whole backward needs ONE
 * correlation C[t] = sum_{b,v} delta[b,v] x[b, v + t - p]:  dL/dK_g = lambda_g C,  dL/dlambda_g = <K_g, C>.
 * ------------------------------------------------------------------------- */

/* C [kz,kx,ky] f32.  gout = dL/dout [B,1,Z,X,Y] f32; when `out` (the forward output, f32) is given,
 * delta = gout * (out > 0) * (1 - out^2) (the relu(tanh) derivative) else delta = gout.  x as in sn_conv_bank.
 * partial_ws: scratch [sn_conv_corr_blocks(B,Z,X,Y), kz*kx*ky] f32; the block partials are summed in a fixed
 * order (bit-reproducible). */
int sn_conv_corr(const void* x, int x_dtype, const float* gout, const float* out, int B, int Z, int X, int Y,
                 int kz, int kx, int ky, float* partial_ws, float* C, sn_stream_t stream);
int sn_conv_corr_blocks(int B, int Z, int X, int Y);
/* The same with gout / out of g_dtype SN_F32 or SN_BF16 (bf16 activations: half the bytes of the two grids this pass
 * reads; the products are formed and summed in fp32 either way). */
int sn_conv_corr_t(const void* x, int x_dtype, const void* gout, const void* out, int g_dtype, int B, int Z, int X, int Y,
                   int kz, int kx, int ky, float* partial_ws, float* C, sn_stream_t stream);

/* The same behind ONE caller-owned workspace of sn_conv_corr_ws_bytes(...) bytes (256-byte aligned), and the entry point
 * that serves binary occupancy (x_dtype SN_OCC8) as a GATHER over the set voxels (K4s, csrc/corr.hip: a list kernel +
 * a gather kernel; no matrix core; nnz x kz kx ky terms instead of V x kz x 256 products): the workspace then also holds
 * the voxel lists.  Any other input, option "corr_dense" = 1, or a workspace with room for the partial rows only
 * (>= sn_conv_corr_blocks x kz kx ky floats) takes sn_conv_corr_t's kernels.  Both forms sum in a fixed order
 * (bit-reproducible per form; the two forms differ by fp32 summation order).  Option "corr_sparse_tile_bytes"
 * (0 = 2048): input bytes per gather job. */
size_t sn_conv_corr_ws_bytes(int x_dtype, int B, int Z, int X, int Y, int kz, int kx, int ky);
int sn_conv_corr_ws(const void* x, int x_dtype, const void* gout, const void* out, int g_dtype, int B, int Z, int X,
                    int Y, int kz, int kx, int ky, void* ws, size_t ws_bytes, float* C, sn_stream_t stream);

/* What sn_conv_corr_ws would launch for these arguments under the options in force now ("corr_dense",
 * "corr_sparse_tile_bytes"), given a workspace of sn_conv_corr_ws_bytes(...) and pointers aligned the way a fresh
 * allocation is: host arithmetic only, from the planners the launches themselves call; no launch, no device.
 * plan8 (8 x int32, host memory):
 *   [0] kernel: 0 the thread-per-tap kernel, 1 the fp32-MFMA GEMM form (K4), 2 the gather over the set voxels (K4s)
 *   [1] input rows per job (the thread-per-tap kernel: x extent of its tile, 8)
 *   [2] row tiles per plane
 *   [3] jobs (the thread-per-tap kernel: tiles)
 *   [4] workgroups launched (persistent for K4 / K4s: job, job + [4], ... run on one workgroup; each writes one partial row)
 *   [5] the kz instantiation of the kernel: 9 (kz <= 9) or 16; 0 for the thread-per-tap kernel
 *   [6] dynamic LDS bytes per workgroup
 *   [7] flags: bit 0 Y admits the four-element staging loads (K4: Y % 4 == 0; K4s: also the delta tile within 4096
 *       elements), bit 1 the list kernel's 8-byte loads (K4s: Y % 8 == 0), bit 2 K4 runs every K step of a non-empty row
 *       (more than 32 steps: Y > 128), bit 3 the gather has more than one group of threads (kx ky <= 256)
 * Returns SN_OK, SN_ERR_INVALID_ARG (null plan8, an extent <= 0, unknown x_dtype / g_dtype) or SN_ERR_UNSUPPORTED where
 * sn_conv_corr_ws returns it (bf16 gradients with a kernel extent > 16, a kernel too large for the thread-per-tap tile).
 * No reference counterpart (autograd has no plan to ask about): what lets tests/test_gpu_corr_plans.py name the fork each
 * of its shapes is there for. */
int sn_conv_corr_plan(int x_dtype, int g_dtype, int B, int Z, int X, int Y, int kz, int kx, int ky, int32_t* plan8);

/* Generator Jacobians: dparams [G, SN_NPARAM] f32 = d<dW, bank(params)>/dparams for dW [G,kz,kx,ky] f32
 * (apex has no gradient: it is truncated to an index, arrow.py:235, and non-trainable, arrow.py:134). */
int sn_geneo_bank_bwd(const float* params, const int32_t* kinds, int G, int kz, int kx, int ky,
                      const float* dW, float* dparams, sn_stream_t stream);

/* The parameter side of SceneNet's backward in one launch, from the correlation C of sn_conv_corr (by linearity
 * dL/dK_g = lambda_g C): dparams [G, SN_NPARAM] as sn_geneo_bank_bwd would give for dW_g = lambda_g C, and
 * dlambdas [G] = <K_g, C> - <K_last, C> -- the gradient of the trainable convex coefficients when coefficient `last`
 * is 1 - sum(others) (SCENE_Net.py:331; entry `last` comes out 0).  bank [G,kz,kx,ky] and lambdas [G] (effective
 * coefficients) are the forward's. */
int sn_geneo_backward(const float* params, const int32_t* kinds, int G, int kz, int kx, int ky, const float* bank,
                      const float* lambdas, const float* corr, int last, float* dparams, float* dlambdas,
                      sn_stream_t stream);

/* ------------------------------------------------------------------------- *
 * K5  training criterion on the prediction grid
 * replaces: WeightedMSE.forward + get_weight_target/get_dens_target (core/criterions/w_mse.py:114-151),
 *           FocalTverskyLoss.forward / TverskyLoss.forward (core/criterions/tversky_loss.py:81-95, :35-51),
 *           BinaryDiceLoss.forward, p = 2, reduction 'mean' (core/criterions/dice_loss.py:33-51),
 *           summed as in GENEO_Loss / GENEO_Dice_Loss / GENEO_Tversky_Loss.forward (geneo_loss.py:72-81, :131-161).
 * The scalar penalties over the ~50 parameters (cvx_loss, positive_regularizer, geneo_loss.py:36-70) stay on the
 * host side.
 *
 * Everything the criterion needs from the B*n_per elements is a handful of sums, taken in ONE pass over
 * (pred, gt): per weight bin k (bin = argmin_k |gt - ranges[k]|, first minimum, w_mse.py:122) the element count and
 * sum (gt - pred)^2; per sample sum p*t, sum p, sum t, sum p^2, sum t^2.  fp64 accumulation, fixed summation order
 * (bit-reproducible).  The weights' mean (w_mse.py:144) is sum_k cnt_k w_k / n.
 * ------------------------------------------------------------------------- */
#define SN_LOSS_MAX_BINS 16
#define SN_LOSS_NSTAT(H) (3 * (H) + 5)   /* cnt[H], sq_err[H], sum_pt, sum_p, sum_t, sum_pp, sum_tt, bce[H] */
#define SN_LOSS_PARTS(n_per) ((n_per) <= 16384 ? 1 : ((n_per) >= 16384 * 256 ? 256 : (int)(((n_per) + 16383) / 16384)))
#define SN_LOSS_WS_DOUBLES(B, n_per, H) ((int64_t)(B) * SN_LOSS_PARTS(n_per) * SN_LOSS_NSTAT(H))
#define SN_LOSS_NCOEF(B) (2 * SN_LOSS_MAX_BINS + 3 * (B))
typedef enum { SN_LOSS_WMSE = 1, SN_LOSS_FOCAL_TVERSKY = 2, SN_LOSS_DICE = 4, SN_LOSS_WBCE = 8 } sn_loss_term;

/* Forward.  pred [B, n_per] (SN_F32 | SN_F64), gt [B, n_per] (SN_F32 | SN_F64 | SN_U8 | SN_OCC8),
 * ranges [H] f32 (left bin edges, w_mse.py:100), bin_w [H] f32 = max(1 - alpha*dens_k, eps) per bin BEFORE the
 * division by the mean (w_mse.py:128-142; ~10 numbers the host derives from the frequency table once).
 * terms = OR of sn_loss_term (SN_LOSS_WBCE = mean(weights * BCELoss(pred, gt)) of BinaryDiceLoss_BCE,
 * core/criterions/dice_loss.py:71-80, with torch's clamps: log >= -100, gradient denominator >= 1e-12).
 * Outputs: stats [B, SN_LOSS_NSTAT(H)] f64; loss [5] f64 = {sum of the requested terms, weighted MSE, focal Tversky,
 * dice, weighted BCE}; coef [SN_LOSS_NCOEF(B)] f64 for sn_loss_backward.
 * parts_ws: scratch [SN_LOSS_WS_DOUBLES(B, n_per, H)] f64. */
int sn_loss_forward(const void* pred, int pred_dtype, const void* gt, int gt_dtype, int B, int64_t n_per,
                    const float* ranges, const float* bin_w, int H, int terms, double mse_weight,
                    double tversky_alpha, double tversky_beta, double focal_gamma, double tversky_smooth,
                    double dice_smooth, double* parts_ws, double* stats, double* loss, double* coef,
                    sn_stream_t stream);

/* The penalties of GENEO_Loss over the model's scalars (core/criterions/geneo_loss.py:36-70) in one launch:
 * value[0] = weight * ( sum_{mask[i] >= 1} relu(-P[i]) + [with_sum] relu(-(1 - sum_{mask[i] == 2} P[i])) ),
 * grad[i] = d value / d P[i].  P [N] f32 (the packed parameter vector), mask [N] i8: 0 = not a parameter,
 * 1 = GENEO parameter (positive_regularizer), 2 = trainable convex coefficient (cvx_loss: its own relu(-phi) and the
 * relu(-(1 - sum)) of the frozen last one).  1 <= N <= 8192 (the launch keeps 8 N bytes in LDS), here and in
 * sn_criterion_forward; SN_ERR_UNSUPPORTED above. */
int sn_param_penalty(const float* P, const int8_t* mask, int N, float weight, int with_sum, float* value, float* grad,
                     sn_stream_t stream);

/* Backward: grad_pred[b,i] = up * (c[bin(gt)] (p - t) + e[bin(gt)] (p - t) / max((1 - p) p, 1e-12) + A_b t + B_b + C_b p),
 * in pred's dtype (c, e, A, B, C from coef).
 * upstream: device scalar f64 (dL/dloss), NULL = 1. */
int sn_loss_backward(const void* pred, int pred_dtype, const void* gt, int gt_dtype, int B, int64_t n_per,
                     const float* ranges, int H, const double* coef, const double* upstream, void* grad_pred,
                     sn_stream_t stream);
/* The same two with what a float32 criterion needs to stay free of cast launches (a training step replayed from a hipGraph
 * pays ~4 us of GPU time for every one-element kernel): sn_loss_forward_m also writes the five losses rounded to float32
 * (loss_f32 [5], nullable); sn_loss_backward_u takes the upstream scalar as SN_F64 or SN_F32. */
int sn_loss_forward_m(const void* pred, int pred_dtype, const void* gt, int gt_dtype, int B, int64_t n_per,
                      const float* ranges, const float* bin_w, int H, int terms, double mse_weight, double tversky_alpha,
                      double tversky_beta, double focal_gamma, double tversky_smooth, double dice_smooth, double* parts_ws,
                      double* stats, double* loss, float* loss_f32, double* coef, sn_stream_t stream);
int sn_loss_backward_u(const void* pred, int pred_dtype, const void* gt, int gt_dtype, int B, int64_t n_per,
                       const float* ranges, int H, const double* coef, const void* upstream, int up_dtype, void* grad_pred,
                       sn_stream_t stream);
/* The criterion of a GENEO_Loss family member (dense terms + cvx_loss + positive_regularizer, geneo_loss.py:36-91, 145-161)
 * in the launches of sn_loss_forward / sn_loss_backward alone: sn_criterion_forward = sn_loss_forward_m with
 * sn_param_penalty's work opening the combine launch, and total_f32 [1] = (float)loss[0] + pen_value -- the scalar the
 * criterion returns; sn_criterion_backward = sn_loss_backward_u with pen_out [N] = pen_grad [N] x upstream riding in the
 * gradient launch.  Same numbers, bit for bit, as the three forward launches + the torch add / multiply they replace. */
int sn_criterion_forward(const void* pred, int pred_dtype, const void* gt, int gt_dtype, int B, int64_t n_per,
                         const float* ranges, const float* bin_w, int H, int terms, double mse_weight, double tversky_alpha,
                         double tversky_beta, double focal_gamma, double tversky_smooth, double dice_smooth,
                         double* parts_ws, double* stats, double* loss, float* loss_f32, double* coef, const float* P,
                         const int8_t* mask, int N, float weight, int with_sum, float* pen_value, float* pen_grad,
                         float* total_f32, sn_stream_t stream);
int sn_criterion_backward(const void* pred, int pred_dtype, const void* gt, int gt_dtype, int B, int64_t n_per,
                          const float* ranges, int H, const double* coef, const void* upstream, int up_dtype,
                          void* grad_pred, const float* pen_grad, int N, float* pen_out, sn_stream_t stream);

/* ------------------------------------------------------------------------- *
 * K20  weighted pinball loss of the quantile ensemble (csrc/quantile.hip)
 * replaces: QuantileLoss.quantile_loss + forward (core/criterions/quant_loss.py:74-102) over
 *           WeightedMSE.get_weight_target (core/criterions/w_mse.py:114-145), which QuantileGENEOLoss.forward
 *           (quant_loss.py:118-142) adds its penalties to.
 *
 * With d = gt[b,v] - pred[b,i,v] and w(gt) = bin_w at K5's bin (argmin_k |gt - ranges[k]|, first minimum, in gt's dtype;
 * byte targets through a 256-entry table):
 *     L = sum_{b,v} w(gt[b,v]) sum_i max(q_i d, (q_i - 1) d)  /  sum_{b,v} w(gt[b,v])
 * -- mean(weights / mean(weights) * sum_i rho_i) over the B * n_per voxels, PER SAMPLE: the reference's
 * `y_gt - y_pred[:, i]` broadcasts a [B,1,...] ground truth against [B,...] to [B,B,...] (every ground truth against every
 * sample's prediction) and is this formula only at B = 1.
 * q_i and q_i - 1 are float32 (the reference holds qs as a float32 tensor); d and rho are evaluated in the promoted type of
 * pred and gt (fp64 when either is SN_F64, else fp32); every sum is fp64 in a fixed order (bit-reproducible).
 * Gradient: dL/dpred[b,i,v] = up * w(gt[b,v]) / sum w * g,  g = -q_i (d > 0), 1 - q_i (d < 0), 0.5 - q_i (d == 0: torch.max
 * hands half of the gradient to each argument at a tie), in pred's dtype.
 * A NaN in pred or gt makes the loss NaN; the gradient at such an element is unspecified.
 *
 * Launch plan: forward = SN_QUANTILE_PARTS(n_per) x B workgroups (K5's: 16384 voxels per part, at most 256 parts) + one
 * combining workgroup; backward = SN_QUANTILE_BWD_PARTS(n_per) x B workgroups (8192 voxels per part, at most 512).  A
 * part spans ceil(n_per / parts) voxels rounded up to a multiple of 4; the 4-wide loop runs when n_per % 4 == 0, the element
 * loop otherwise.  No atomics, no allocation; capturable.
 * ------------------------------------------------------------------------- */
#define SN_QUANTILE_MAX_Q 8
#define SN_QUANTILE_PARTS(n_per) SN_LOSS_PARTS(n_per)
#define SN_QUANTILE_BWD_PARTS(n_per) ((n_per) <= 8192 ? 1 : ((n_per) >= 8192 * 512 ? 512 : (int)(((n_per) + 8191) / 8192)))
#define SN_QUANTILE_NSTAT(Q, H) ((Q) + (H))   /* sum_v w rho_i [Q], count of bin k [H] */
#define SN_QUANTILE_WS_DOUBLES(B, n_per, Q, H) ((int64_t)(B) * SN_QUANTILE_PARTS(n_per) * SN_QUANTILE_NSTAT(Q, H))

/* Forward.  pred [B, Q, n_per] (SN_F32 | SN_F64), gt [B, n_per] (SN_F32 | SN_F64 | SN_U8 | SN_OCC8), qs [Q] HOST floats
 * (passed to the kernels by value), ranges / bin_w [H] f32 as in sn_loss_forward.
 * Outputs: loss [1 + Q] f64 = {L, each quantile's share of it}; loss_f32 [1 + Q] (nullable) the same rounded once;
 * coef [H] f64 = bin_w[k] / sum w for sn_quantile_backward; stats [B, SN_QUANTILE_NSTAT(Q, H)] f64 (per sample: the Q
 * weighted pinball sums, then the H bin counts).  parts_ws: scratch [SN_QUANTILE_WS_DOUBLES(B, n_per, Q, H)] f64.
 * SN_ERR_INVALID_ARG: a null pointer, B <= 0, n_per <= 0, Q outside 1..SN_QUANTILE_MAX_Q, H outside 1..SN_LOSS_MAX_BINS, an
 * unknown dtype, a misaligned pointer (n_per % 4 == 0: 16 bytes, byte gt 4);  SN_ERR_UNSUPPORTED: SN_BF16 predictions, a q
 * outside (0, 1), B > 65535.  All checked before any launch. */
int sn_quantile_forward(const void* pred, int pred_dtype, const void* gt, int gt_dtype, int B, int Q, int64_t n_per,
                        const float* qs, const float* ranges, const float* bin_w, int H, double* parts_ws, double* stats,
                        double* loss, float* loss_f32, double* coef, sn_stream_t stream);
/* Backward: grad_pred [B, Q, n_per] in pred's dtype, one launch.  upstream: device scalar SN_F64 | SN_F32 (dL/dloss),
 * NULL = 1.  Checks as sn_quantile_forward. */
int sn_quantile_backward(const void* pred, int pred_dtype, const void* gt, int gt_dtype, int B, int Q, int64_t n_per,
                         const float* qs, const float* ranges, int H, const double* coef, const void* upstream,
                         int up_dtype, void* grad_pred, sn_stream_t stream);


/* ---------------------------------------------------------------------------
 * K6 -- training metrics (csrc/metrics.hip)
 * replaces: the torchmetrics 0.9 MetricCollection of init_metrics(tau) (utils/scripts_utils.py:80-91) that
 *           LitSceneNet.{training,validation,test}_step call on every batch (core/lit_modules/lit_model_wrappers.py).
 *
 * One call counts a flattened binary prediction against its target:
 *   predicted positive: pred >= tau in pred's dtype (tau rounded to it: fp32 0.65 -> 0.64999998f, bf16 -> 0.6484375);
 *                       NaN is negative
 *   target positive:    int(target) == 1 under C truncation (0.999 -> 0, 1.7 -> 1); a target whose truncation is
 *                       neither 0 nor 1 (>= 2, <= -1, NaN, +-Inf, bytes > 1) is a BAD target
 *   bad pred:           pred < 0 || pred > 1 (torchmetrics raises on it; the caller reads the counter)
 * counts [SN_METRIC_NCOUNT] u64 = tp, fp, fn, tn, bad_pred, bad_target.
 * values [SN_METRIC_NVALUE] f32 = JaccardIndex (macro mean of the two classes' IoU), Precision, Recall, F1Score,
 * FBetaScore, computed in fp64 from the counts, 0/0 -> 0.
 * ------------------------------------------------------------------------- */
#define SN_METRIC_NCOUNT 6          /* tp, fp, fn, tn, bad_pred, bad_target */
#define SN_METRIC_NVALUE 5          /* JaccardIndex, Precision, Recall, F1Score, FBetaScore */
#define SN_METRIC_MAX_PARTS 1024
#define SN_METRIC_WS_BYTES (SN_METRIC_MAX_PARTS * SN_METRIC_NCOUNT * 8)

/* pred [n] SN_F32 | SN_BF16 | SN_F64; target [n] SN_F32 | SN_F64 | SN_BF16 | SN_U8 | SN_OCC8 | SN_I32 (element-aligned
 * pointers suffice: an unaligned head and tail are counted element by element).  tau in (0, 1), beta > 0.
 * parts_ws: scratch of SN_METRIC_WS_BYTES (8-byte aligned).  state [NCOUNT] u64: caller-owned, ACCUMULATES this call's
 * counts; batch [NCOUNT] u64 (nullable): this call's counts; values [2 x NVALUE] f32 (nullable): this call's values,
 * then the values of the accumulated state.  Two launches (counting pass, one-workgroup combine), no atomics, no
 * allocation, no synchronisation: capturable; the counts do not depend on launch order. */
int sn_binary_stats(const void* pred, int pred_dtype, const void* target, int target_dtype, int64_t n, double tau,
                    double beta, void* parts_ws, uint64_t* state, uint64_t* batch, float* values, sn_stream_t stream);

/* K6 at T thresholds in one pass: the precision-recall curve's counts.
 * replaces: the BinnedAveragePrecision(num_classes=1, thresholds=torch.linspace(0.5, 0.95, 20)) that the reference's
 *           MetricCollection carries commented out (utils/scripts_utils.py:90), and T calls of sn_binary_stats.
 *
 * pred / target hold S equal segments of n elements each (S = 1: the whole batch; S = B, n = Z*X*Y: one curve per
 * tile); dtypes and the element-alignment rule are sn_binary_stats'.  thresholds_host [T] fp64, HOST memory, read during
 * the call only (they travel as kernel arguments: a captured replay keeps those of capture time), strictly increasing,
 * inside (0, 1), 1 <= T <= SN_CURVE_MAX_THRESHOLDS.  Each is rounded to pred's dtype the way sn_binary_stats rounds tau;
 * two that round to the same value are legal and give equal columns.
 * Per segment, bin(p) = number of rounded thresholds <= p, in 0..T (NaN: 0), and a record of
 * SN_CURVE_RECORD(T) = 2 * (T + 1) + 2 u64:  hist[2][T + 1] (target negative, then positive), bad_pred, bad_target.
 * For every k the counts sn_binary_stats gives for that segment at tau = thresholds[k] are
 *   tp = sum_{b > k} hist[1][b], fp = sum_{b > k} hist[0][b], fn = sum hist[1] - tp, tn = sum hist[0] - fp,
 * and bad_pred / bad_target are its counters (they do not depend on the threshold).
 * state [S][SN_CURVE_RECORD(T)] u64: caller-owned, ACCUMULATES this call's records; batch (nullable, same shape): this
 * call's records.  parts_ws: scratch of ws_bytes >= sn_binary_curve_ws_bytes(n, S, T) (0 for a shape the entry refuses),
 * 8-byte aligned.  S <= 2^20, S * n <= 2^40.  Two launches (histogram pass, combine), LDS integer adds inside a workgroup
 * only, plain stores, no allocation, no synchronisation: capturable, and independent of launch order. */
#define SN_CURVE_MAX_THRESHOLDS 255
#define SN_CURVE_RECORD(T) (2 * ((T) + 1) + 2)
size_t sn_binary_curve_ws_bytes(int64_t n, int S, int T);
int sn_binary_curve(const void* pred, int pred_dtype, const void* target, int target_dtype, int64_t n, int S,
                    const double* thresholds_host, int T, void* parts_ws, size_t ws_bytes, uint64_t* state,
                    uint64_t* batch, sn_stream_t stream);


/* ------------------------------------------------------------------------- *
 * K7 -- tile ingest: the raw rows of a batch of tiles -> the pts / labels layout of K1 and sn_gather_points.
 * replaces: the per-sample split on the host, core/datasets/ts40k.py:201-207 (`npy = np.load(...)`,
 *           `sample = (npy[:, 0:-1], npy[:, -1])`; tiles.split_tile + pack_csr here): a file's rows go host-to-device
 *           as they are and are de-interleaved on the device.
 * ------------------------------------------------------------------------- */

/* rows [total, cols] row-major of row_dtype (SN_F64 | SN_F32): the raw rows of B tiles, concatenated (element-aligned).
 * pts [total,3] f64 = columns 0..2; labels (nullable) [total] f64 = column cols-1.  3 <= cols <= 8; labels need cols >= 4.
 * f64 rows: every 64-bit pattern is carried unchanged (NaN payloads, -0.0, denormals).  f32 rows: the exact widening (a
 * NaN keeps sign and payload and gets the quiet bit).  Nothing beyond `total` is written.  With cols == 4 and rows, pts,
 * labels 16-byte aligned the kernel moves two points per lane with 16-byte accesses; otherwise one point per lane.
 * bad (nullable) [B] i32, WRITTEN (not accumulated) by the call: points of tile b with a non-finite value in a column
 * that is read (x, y, z; the label column only when labels is given); needs offsets [B+1] i64 (device, CSR).  offsets
 * may be null iff bad is null.  A memset node (bad only) and one launch; integer atomics for the non-finite points only:
 * no allocation, no synchronisation, capturable, independent of launch order.
 * SN_ERR_INVALID_ARG: null rows / pts, total <= 0, B <= 0, cols outside 3..8, labels with cols == 3, bad without offsets,
 * an unknown dtype, a misaligned pointer;  SN_ERR_UNSUPPORTED: a known dtype other than SN_F32 / SN_F64. */
int sn_tiles_unpack(const void* rows, int row_dtype, int cols, int64_t total, const int64_t* offsets, int B,
                    double* pts, double* labels, int32_t* bad, sn_stream_t stream);


/* ------------------------------------------------------------------------- *
 * K8 -- tower proposals: DBSCAN over the voxels of a thresholded prediction, on the device.
 * replaces: eda.extract_towers (utils/pcd_processing.py:577-651: open3d's cluster_dbscan and a pandas group-by, one tile
 *           at a time on the host) behind prob_to_label (utils/voxelization.py:304-323) and vxg_to_xyz, as extract_towers,
 *           compute_euc_dists and get_tower_proposals call it with eps = 3.5, min_points = 18
 *           (utils/observer_utils.py:397-473, 556-); the statistics rows carry what filter_towers (:503-549) and
 *           aggregate_centroids (:476-500) read from the clusters.
 *
 * grid [B, n0, n1, n2] (the project's grids are [.., nz, nx, ny]: axis 0 is z); tiles are independent.
 *   positive: grid >= tau in the grid's own dtype (tau rounded to it as sn_binary_stats rounds it); NaN is not positive;
 *             SN_U8 / SN_OCC8: non-zero, tau ignored
 *   stencil:  the offsets (d0, d1, d2) with (d0 s0)^2 + (d1 s1)^2 + (d2 s2)^2 <= eps^2, in fp64 in exactly this form,
 *             s = voxel_size per grid axis (null: 1, 1, 1); inclusive; (0, 0, 0) belongs to it; at most 10 voxels per axis
 *   core:     positive, and at least min_points positives of its own tile inside its stencil (clipped at the grid faces)
 *   cluster:  a connected component of the cores under stencil adjacency; ids 0..K-1 ascend with each cluster's smallest
 *             core voxel (linear index in memory order)
 *   border:   positive, not core, a core inside its stencil: takes the smallest id among those cores
 *   labels:   the id, -1 for everything else
 * ------------------------------------------------------------------------- */
#define SN_TOWER_NSTAT 12   /* n_voxels, n_core, sum_i0, sum_i1, sum_i2, min_i0, min_i1, min_i2, max_i0, max_i1, max_i2, first_core_index */
#define SN_TOWER_LAUNCHES 6 /* threshold, core, union, flatten, rank, finish */

/* The stencil's rows: rows_host [cap, 3] receives (d0, d1, half-width along axis 2) of the first `cap` rows, ascending in
 * (d0, d1) (null: none); n_offsets (nullable) the number of offsets, sum of 2 * half-width + 1.  Host only, no GPU.
 * Returns the row count (>= 1); SN_ERR_INVALID_ARG for eps or a voxel size that is not positive and finite;
 * SN_ERR_UNSUPPORTED when eps reaches more than 10 voxels along an axis. */
int sn_towers_stencil(double eps, const double* voxel_size_host, int32_t* rows_host, int cap, int64_t* n_offsets);

/* Workspace bytes of one sn_tower_proposals call: 0 for a shape the entry refuses (an extent <= 0, more than 2^24 voxels
 * per tile or 2^36 per call, rows counted as padded to a multiple of 64; more than 65535 tiles). */
size_t sn_towers_ws_bytes(int B, int n0, int n1, int n2);

/* grid: SN_F32 | SN_BF16 | SN_F64 | SN_U8 | SN_OCC8, element-aligned.  tau in (0, 1) for the float dtypes; eps > 0 and
 * finite; voxel_size_host: 3 doubles in HOST memory or null, read during the call only (the stencil travels as a kernel
 * argument: a captured replay keeps that of capture time); min_points >= 1; max_towers >= 0.
 * ws: caller-owned scratch of ws_bytes >= sn_towers_ws_bytes(...), 8-byte aligned.
 * labels [B, n0, n1, n2] i32: always the full ids.  n_towers [B] i32: the true K, also when K > max_towers.
 * stats [B, max_towers, SN_TOWER_NSTAT] i64 (null iff max_towers == 0): rows of the ids below max_towers, over every
 * voxel that carries the id (cores and borders; n_core counts the cores); rows of absent clusters are zero.
 * SN_TOWER_LAUNCHES launches on `stream`; lock-free union-find (compare-and-swap on parents that only decrease), no
 * workgroup waits for another; integer atomics only: results do not depend on scheduling.  No allocation, no
 * synchronisation: capturable.
 * SN_ERR_INVALID_ARG: a null pointer, B or an extent <= 0, min_points < 1, eps <= 0 or not finite, tau outside (0, 1)
 * for a float grid, max_towers < 0, a short workspace, a misaligned pointer, an unknown dtype;  SN_ERR_UNSUPPORTED: a known
 * dtype that is no grid dtype (SN_I32), eps beyond 10 voxels along an axis, a shape sn_towers_ws_bytes refuses. */
int sn_tower_proposals(const void* grid, int dtype, int B, int n0, int n1, int n2, double tau, double eps,
                       const double* voxel_size_host, int min_points, int max_towers, void* ws, size_t ws_bytes,
                       int32_t* labels, int32_t* n_towers, int64_t* stats, sn_stream_t stream);

/* DIAGNOSTIC entry, no part of the stable interface: the launches first..last (1-based, of SN_TOWER_LAUNCHES) of the same
 * call and nothing else.  tools/towers_bench.py times the prefixes 1..k through it and takes differences.  The number
 * and order of the launches may change with the kernels; launches left out must have run before on the same workspace. */
int sn_tower_proposals_launches(const void* grid, int dtype, int B, int n0, int n1, int n2, double tau, double eps,
                                const double* voxel_size_host, int min_points, int max_towers, void* ws, size_t ws_bytes,
                                int32_t* labels, int32_t* n_towers, int64_t* stats, int first, int last,
                                sn_stream_t stream);


/* ------------------------------------------------------------------------- *
 * K9 -- scan crops: K disc / box regions cut out of one scan into a CSR batch of K tiles, on the device.
 * replaces: the host-side crops of utils/pcd_processing.py -- crop_at_locations (:820-840), crop_tower_radius (:666-697),
 *           crop_two_towers (:700-739) and crop_tower_samples (:805-817), which core/datasets/ts40k.py:31-148
 *           build_data_samples drives: each an `a[mask]` over the whole cloud, once per centre.
 *
 * scan:     pts [n,3] f64 (x, y, z), labels [n] f64 or null -- the layout of K1 and K7
 * regions:  regions [K,4] f64 and kinds [K] i32 (null: all discs), both on the DEVICE
 *   SN_CROP_DISC  row (cx, cy, r, unused): point i is a member iff (x-cx)*(x-cx) + (y-cy)*(y-cy) <= r*r, evaluated in fp64
 *                 in exactly this form, each product and the sum rounded once and never contracted -- what
 *                 np.sum(np.power(xyz[:, :2] - c[:2], 2), axis=1) <= radius*radius computes.  z takes no part.
 *   SN_CROP_BOX   row (xmin, ymin, xmax, ymax): a member iff xmin <= x && x <= xmax && ymin <= y && y <= ymax (inclusive on
 *                 both ends, z disregarded: crop_two_towers)
 *   The comparisons are taken literally: a NaN x or y is in no region; r NaN gives an empty region; a negative r behaves
 *   as |r|; r = +inf admits every point whose dx, dy are not NaN; a box with min > max is empty; -inf <= -inf is true.
 *   A kinds value other than 0 or 1 makes that region EMPTY (it lives in device memory: no entry can refuse it).
 * output:   a CSR batch of K tiles.  offsets [K+1] i64 holds the TRUE sizes, whatever the capacity.  Tile k holds the
 *           members of region k in scan order (stable): scan[mask_k] row for row.  Overlapping or repeated regions repeat
 *           rows.  x, y, z and the label are moved as 64-bit patterns (NaN payloads, -0.0, denormals unchanged, as K7).
 *           src [total] i64 (nullable): each output row's index in the scan.
 * ------------------------------------------------------------------------- */
#define SN_CROP_DISC 0
#define SN_CROP_BOX 1

/* Workspace bytes of sn_crop_count / sn_crop_scatter: 8 * K * (chunks + 1), chunks = ceil(n / sn_crops_chunk_points()).
 * 0 for a shape the entries refuse (n <= 0, K <= 0, n > 2^36, K > 65536). */
size_t sn_crops_ws_bytes(int64_t n, int K);
/* Points per workgroup (1024): host only -- lets a test put its sizes on the seams. */
int sn_crops_chunk_points(void);

/* Member counts of every (region, workgroup) into ws, their exclusive prefixes per region in place, and offsets [K+1].
 * Three launches on `stream` (count, prefix, offsets); every slot is written by exactly one workgroup: no memset, no
 * atomics, no workgroup waits for another.  No allocation, no synchronisation: capturable; results do not depend on
 * scheduling.
 * SN_ERR_INVALID_ARG: a null pts / regions / ws / offsets, n <= 0, K <= 0, ws_bytes < sn_crops_ws_bytes(n, K), a
 * misaligned pointer (8 bytes; kinds 4);  SN_ERR_UNSUPPORTED: n > 2^36 or K > 65536. */
int sn_crop_count(const double* pts, int64_t n, const double* regions, const int32_t* kinds, int K, void* ws,
                  size_t ws_bytes, int64_t* offsets, sn_stream_t stream);

/* Called with the same pts / regions / kinds and the ws / offsets that sn_crop_count left: writes output row
 * offsets[k] + rank of every member whose output index is < capacity -- out_pts [capacity,3], out_labels [capacity] (null
 * iff labels is null), out_src [capacity] (nullable).  Rows at or beyond capacity and everything beyond offsets[K] are NOT
 * touched.  The test is recomputed, for the regions whose count says the workgroup's points hold a member.  One launch;
 * no allocation, no synchronisation: capturable.
 * SN_ERR_INVALID_ARG: as sn_crop_count, and a null out_pts, capacity < 0, out_labels without labels or the reverse;
 * SN_ERR_UNSUPPORTED: as sn_crop_count. */
int sn_crop_scatter(const double* pts, const double* labels, int64_t n, const double* regions, const int32_t* kinds, int K,
                    const void* ws, size_t ws_bytes, const int64_t* offsets, int64_t capacity, double* out_pts,
                    double* out_labels, int64_t* out_src, sn_stream_t stream);


/* ------------------------------------------------------------------------- *
 * K12 -- region census: what the labels inside each of K9's regions are, before anything is cut.
 * replaces: the per-candidate crop, read-back and numpy pass by which the reference decides whether a region becomes a
 *           sample -- crop_ground_samples (utils/pcd_processing.py:742-762: more than 300 points, at least two classes,
 *           no tower), build_pole_samples (core/datasets/semKITTI.py:37-88: at least 5 pole points per slab),
 *           build_pole_radius_samples (:105-158: at least 5 per disc) and the scan-level gates np.any(classes == TOWER)
 *           (ts40k.py:88) / np.any(gt == pole_label) (semKITTI.py:142).
 *
 * scan, regions, kinds: as K9, and MEMBERSHIP IS K9's, bit for bit (the same device function): the disc and box tests of
 *           the K9 block, kinds null = all discs, any other kind an empty region, a NaN x or y in no region.
 * watch:    [C,2] f64 on the device, C <= SN_CENSUS_MAX_WATCH inclusive ranges (lo, hi) of label values
 * output:   counts [K, 2 + C] i64:  [k][0] members;  [k][1] members whose label is NaN (0 without labels);
 *           [k][2 + c] members with watch[c][0] <= label && label <= watch[c][1], taken literally: a NaN label or a NaN
 *           bound never matches.  Equality with v is (v, v); trunc(label) == v for v > 0 is (v, nextafter(v + 1, -inf)).
 *           label_range [K,2] f64: (min, max) over the members' labels that are not NaN, in the order that puts -0.0 below
 *           +0.0 -- a definite bit pattern; (+inf, -inf) for a region with no such member.
 *           "At least two distinct label values" as np.unique counts them (all NaNs one value) is
 *           min < max || (n_nan > 0 && n_nan < n).
 *           Every output is an integer sum or a maximum of integer codes: it does not depend on scheduling.
 * ------------------------------------------------------------------------- */
#define SN_CENSUS_MAX_WATCH 16

/* Workspace bytes of sn_crop_census: 8 * 8 * K * (C + 4) -- eight shards of K rows of C + 4 words.  0 for a shape the entry refuses (n <= 0, K <= 0, n > 2^36,
 * K > 65536, C < 0, C > SN_CENSUS_MAX_WATCH). */
size_t sn_crop_census_ws_bytes(int64_t n, int K, int C);
/* Points per workgroup of the census kernel (1024): host only -- lets a test put its sizes on the seams. */
int sn_census_chunk_points(void);

/* One memset node over ws and two launches on `stream`: the census (one wave per sn_census_chunk_points() points; what a
 * workgroup finds is reduced over the wave and added to the region's row in one of ws' eight shards by 64-bit integer atomic add / max, only
 * where it is not zero) and a decode that folds the shards into counts and label_range.  No floating-point atomics, no workgroup waits
 * for another, no allocation, no synchronisation: capturable.
 * SN_ERR_INVALID_ARG: a null pts / regions / ws / counts, n <= 0, K <= 0, C < 0, C > 0 without labels, watch given with
 * C == 0 or missing with C > 0, label_range given without labels or missing with them, ws_bytes <
 * sn_crop_census_ws_bytes(n, K, C), a misaligned pointer (8 bytes; kinds 4);
 * SN_ERR_UNSUPPORTED: n > 2^36, K > 65536 or C > SN_CENSUS_MAX_WATCH. */
int sn_crop_census(const double* pts, const double* labels, int64_t n, const double* regions, const int32_t* kinds, int K,
                   const double* watch, int C, void* ws, size_t ws_bytes, int64_t* counts, double* label_range,
                   sn_stream_t stream);


/* ------------------------------------------------------------------------- *
 * K10 -- point DBSCAN: the towers of a labelled scan, on the device.
 * replaces: select_object -> extract_towers (utils/pcd_processing.py:508-522, 577-651: np.isin over the classes, open3d's
 *           cluster_dbscan(eps=10, min_points=300) over the tower points of a whole scan and a pandas group-by, on the
 *           host) in front of crop_tower_samples and crop_two_towers_samples (:765-817), hence of build_data_samples
 *           (core/datasets/ts40k.py:86-92).
 *
 * inputs:    pts [n,3] f64; optionally labels [n] f64 and keep [n_keep] f64: a point is selected iff label == keep[j] for
 *            some j (np.isin: a NaN label is never selected); without labels every point is selected
 * positions: the selected points keep scan order; their positions 0..m-1 are what "index" means below
 * neighbour: q is a neighbour of p iff (dx*dx + dy*dy) + dz*dz <= eps*eps in fp64, in exactly this form, each product and
 *            sum rounded once and never contracted; p is its own neighbour.  The comparison is literal: a point with a NaN
 *            or infinite coordinate is nobody's neighbour, not even its own, and ends as noise
 * core:      a point with at least min_points neighbours
 * cluster:   a connected component of the cores under the neighbour relation; ids 0..K-1 ascend with each cluster's
 *            smallest core position
 * border:    a point that is not core and has a core neighbour: takes the smallest id among its core neighbours
 * noise:     everything else, labelled -1
 * (sklearn.cluster.DBSCAN(algorithm='kd_tree') gives these labels, borders included, on sets without a pair on the rim;
 * open3d's boundary rule and its choice for a border two clusters reach could not be checked and are unpinned, as for K8.)
 * ------------------------------------------------------------------------- */
#define SN_DBSCAN_NSTAT 3      /* n_points, n_core, first core's scan index */
#define SN_DBSCAN_LAUNCHES 8   /* cells, prefix, scatter, core, union, flatten, rank, finish */

/* Scan points per workgroup of sn_points_select (1024) and positions per workgroup of sn_dbscan_points (256): host only
 * -- they let a test put its sizes on the seams. */
int sn_points_select_chunk_points(void);
int sn_dbscan_chunk_points(void);

/* Workspace bytes of sn_points_select over n points (56 per 1024 points); 0 for n <= 0 or n > 2^33. */
size_t sn_points_select_ws_bytes(int64_t n);

/* sel [capacity] i64 (null iff capacity == 0): the scan indices of the selected points, ascending -- scan order by
 * construction (ballot and mbcnt ranks, as K9).  n_sel [1] i64: the TRUE count whatever the capacity; rows at or beyond
 * capacity are not touched.  bbox [6] f64 = (xmin, ymin, zmin, xmax, ymax, zmax) over the selected points' finite
 * coordinates, each axis by itself (+inf, -inf where there is none).  labels null: every point is selected, keep is not
 * read.  keep lives on the DEVICE.  Three launches (count, prefix, scatter), every slot written by one workgroup: no
 * atomics, no allocation, no synchronisation: capturable.
 * SN_ERR_INVALID_ARG: a null pts / ws / n_sel / bbox, labels without keep, n <= 0, n_keep < 0, capacity < 0, sel null with
 * capacity > 0, a short workspace, a pointer not 8-byte aligned;  SN_ERR_UNSUPPORTED: n > 2^33, n_keep > 64. */
int sn_points_select(const double* pts, const double* labels, int64_t n, const double* keep, int n_keep, int64_t capacity,
                     void* ws, size_t ws_bytes, int64_t* sel, int64_t* n_sel, double* bbox, sn_stream_t stream);

/* The search grid of sn_dbscan_points: cubic cells of side k * eps (times 1 + 2^-20, so that rounding of a cell index can
 * never put two neighbours two cells apart) over bounds_host = (xmin, ymin, zmin, xmax, ymax, zmax), dims = floor(extent /
 * side) + 1 per axis, with the smallest integer k >= 1 whose grid has at most max_cells cells.  dims_out [3] i32 and
 * side_out [1] (both nullable).  Host only, no GPU.
 * SN_ERR_INVALID_ARG: null bounds, eps <= 0 or not finite, max_cells < 1, a bound that is not finite, max < min;
 * SN_ERR_UNSUPPORTED: eps outside 1e-150 .. 1e150, max_cells > 2^22. */
int sn_dbscan_cell_grid(const double* bounds_host, double eps, int64_t max_cells, int32_t* dims_out, double* side_out);

/* Workspace bytes of sn_dbscan_points for `capacity` positions and `cells` grid cells (48 B per position, 8 B per cell);
 * 0 for what the entry refuses (capacity < 1 or >= 2^31, cells < 1 or > 2^22). */
size_t sn_dbscan_ws_bytes(int64_t capacity, int64_t cells);

/* Clusters the first min(n_sel, capacity) selected positions of pts [n,3].  sel [>= capacity] i64: their scan indices
 * (null: the identity over the scan's n rows; an index outside 0..n-1 reads as a NaN point); n_sel [1] i64 on the DEVICE
 * (null allowed with a null sel: n).  bounds_host, eps, max_cells: the grid of sn_dbscan_cell_grid, read during the call
 * only (it travels as a kernel argument: a captured replay keeps that of capture time).  A point outside the bounds or
 * with a non-finite coordinate is clamped into an edge cell; clamping never moves two cells apart that were adjacent, so
 * the result is exact for ANY bounds -- they only decide the speed.
 * cluster [capacity] i32: one label per position, rows at or beyond min(n_sel, capacity) not touched.  n_clusters [1] i32:
 * the true K, never clipped.  stats [max_clusters, SN_DBSCAN_NSTAT] i64 (null iff max_clusters == 0): rows of the ids
 * below max_clusters, zero rows for absent ones.  status [1] i32, WRITTEN by the call: bit 0 iff n_sel > capacity.
 * ws: caller-owned scratch of ws_bytes >= sn_dbscan_ws_bytes(capacity, cells of the grid), 16-byte aligned.
 * A memset node and SN_DBSCAN_LAUNCHES launches on `stream`; lock-free union-find over positions (compare-and-swap on
 * parents that only decrease), every loop bounded by the data, no workgroup waits for another; integer atomics only:
 * results do not depend on scheduling.  No allocation, no synchronisation: capturable.
 * SN_ERR_INVALID_ARG: a null pts / ws / cluster / n_clusters / status / bounds, sel without n_sel, n <= 0, capacity <= 0,
 * min_points < 1, eps <= 0 or not finite, max_clusters < 0, stats null with max_clusters > 0, what sn_dbscan_cell_grid
 * calls invalid, a short workspace, a misaligned pointer;  SN_ERR_UNSUPPORTED: capacity >= 2^31, n > 2^33, max_clusters >
 * 2^20, what sn_dbscan_cell_grid calls unsupported. */
int sn_dbscan_points(const double* pts, int64_t n, const int64_t* sel, const int64_t* n_sel, int64_t capacity,
                     const double* bounds_host, double eps, int min_points, int64_t max_cells, int max_clusters, void* ws,
                     size_t ws_bytes, int32_t* cluster, int32_t* n_clusters, int64_t* stats, int32_t* status,
                     sn_stream_t stream);

/* DIAGNOSTIC entry, no part of the stable interface: the launches first..last (1-based, of SN_DBSCAN_LAUNCHES) of the same
 * call and nothing else; tools/dbscan_bench.py times the prefixes 1..k through it and takes differences.  Launches left
 * out must have run before on the same workspace. */
int sn_dbscan_points_launches(const double* pts, int64_t n, const int64_t* sel, const int64_t* n_sel, int64_t capacity,
                              const double* bounds_host, double eps, int min_points, int64_t max_cells, int max_clusters,
                              void* ws, size_t ws_bytes, int32_t* cluster, int32_t* n_clusters, int64_t* stats,
                              int32_t* status, int first, int last, sn_stream_t stream);


/* ------------------------------------------------------------------------- *
 * K11 -- tower scores: K8's statistics rows filtered, merged and matched against the ground truth's towers, on the device.
 * All arithmetic is fp64, each operation rounded once, in exactly the written order (built with -ffp-contract=off; sqrt is
 * the correctly rounded one).
 *
 * Inputs per tile b: stats[b, 0..K-1, SN_TOWER_NSTAT] and n_towers[b] of sn_tower_proposals.  Row i is PRESENT if
 * i < min(n_towers[b], K) and n_voxels > 0.  s = voxel size per grid axis (null: 1, 1, 1; each finite and > 0),
 * h = height_axis in {0, 1, 2}, (p0, p1) the other two axes, ascending.
 *   centroid    c_a = ((double)sum_a / (double)n_voxels) * s_a
 *   extent      e_a = (double)max_a * s_a - (double)min_a * s_a
 *   planar row  q_i = (c_p0, c_p1)
 * (with s = 1 these are TowerProposals.towers(b)'s centroids and box differences bit for bit)
 *
 * Filter (apply_filter != 0; sna.filter_towers):
 *   keep_i = ((e_h >= tower_height) || (max(e_p0, e_p1) <= threshold))
 *            && ((c_p0 - ctr_p0)*(c_p0 - ctr_p0) + (c_p1 - ctr_p1)*(c_p1 - ctr_p1) <= rim_sq)
 *   rim_sq is passed as a number: the caller evaluates (radius - threshold * 2) ** 2 the way the host mirror does (Python's
 *   ** is libm's pow, not always x*x, so the square is never recomputed here).  ctr: three host doubles in scaled units.
 *   apply_filter == 0: every present row is kept (compute_euc_dists' form).
 *
 * Aggregate (sna.aggregate_centroids): over the kept rows in id order, for each i the members are the kept j with
 *   sqrt(dx*dx + dy*dy) <= min_euc, dx = q_j0 - q_i0, dy = q_j1 - q_i1 (the sum in that order); mean_i is the members' rows
 *   added one after another in ascending j starting from 0.0, per column, then divided by (double)count -- numpy's order for
 *   np.mean(axis=0).  agg[b] holds the distinct mean_i rows (numeric equality on both columns) sorted ascending by column 0,
 *   then column 1 (np.unique(axis=0)); n_agg[b] rows are valid, the rest NaN.  The relation is deliberately not transitive:
 *   a chain A-B-C with A, C further apart than min_euc has three different means and gives three rows.
 *
 * Match (compute_euc_dists; neither a filter nor an aggregation on the ground-truth side): for each present ground-truth
 *   row k with planar row g_k (same coordinate rule on gt_stats):
 *   d_m = sqrt((g_k0 - a_m0)*(g_k0 - a_m0) + (g_k1 - a_m1)*(g_k1 - a_m1)) over m < n_agg; match[b,k] is the first m of the
 *   smallest d_m, dist[b,k] that d_m.  n_agg == 0: match = -1, dist = 0.0 (the reference's (gt_c, None, 0)).  Absent rows:
 *   match = -1, dist = NaN.
 *
 * Status: status[b] bit 0 is set when n_towers[b] > K: rows are missing, the outputs cover the rows that exist.
 *
 * Totals: int64[SN_TSCORE_NTOTAL], accumulated into, never zeroed by the call:
 *   tiles, tiles_skipped, gt_towers, proposals (sum of n_agg), hits (match >= 0 && dist <= hit_dist),
 *   misses (gt_towers - hits), false_proposals (aggregated rows that are the match of no hit), one reserved 0.
 *   A tile with bit 0 set on either side adds 1 to tiles_skipped and nothing else.
 * dist_total: one fp64; the sum of the hits' dist is added to it, deterministically (identical bits for identical inputs
 *   and prior contents): no fp atomics, a per-tile partial in row order and a fixed-shape reduction over the tiles in a
 *   second small launch.  It may differ from the tile-order sum by at most hits * 2^-53 * sum(dist), the bound of any
 *   summation order.
 *
 * Not mirrored: get_tower_proposals' "remove buggy centroid" step (utils/observer_utils.py:567-572) drops one cluster whose
 * centroid is exactly (0, 0, 0).  That can only be the single voxel (0, 0, 0), which no min_points >= 2 produces.
 * ------------------------------------------------------------------------- */
#define SN_TSCORE_MAX_ROWS 1024   /* rows per tile either entry serves (the tile's planar rows live in LDS) */
#define SN_TSCORE_NTOTAL 8        /* tiles, tiles_skipped, gt_towers, proposals, hits, misses, false_proposals, reserved */

/* replaces: filter_towers (utils/observer_utils.py:503-549) and aggregate_centroids (:476-500) as get_tower_proposals
 *           (:556-582) chains them behind extract_towers, and the aggregation loop inside compute_euc_dists (:441-454);
 *           here on K8's statistics rows, without the per-tile copy of the label grid that TowerProposals.towers(b) needs.
 * stats [B, max_towers, SN_TOWER_NSTAT] i64, n_towers [B] i32 (device).  voxel_size_host (nullable), center_host (needed
 * with apply_filter): 3 doubles in HOST memory, read during the call only (they travel as kernel arguments: a captured
 * replay keeps capture-time values).
 * keep [B, K] u8: 1 for kept rows.  planar [B, K, 2] f64 (nullable): q of the present rows, NaN absent.  agg [B, K, 2] f64,
 * n_agg [B] i32, status [B] i32 as defined above.
 * One launch, one workgroup per tile, no atomics; no allocation, no synchronisation: capturable.
 * SN_ERR_INVALID_ARG: a null required pointer, B <= 0, max_towers < 1, height_axis outside 0..2, a voxel size or min_euc
 * that is not finite and positive, center_host null with apply_filter, a misaligned pointer;  SN_ERR_UNSUPPORTED: max_towers
 * > SN_TSCORE_MAX_ROWS, B > 65535.  All checked before the launch. */
int sn_tower_centroids(const int64_t* stats, const int32_t* n_towers, int B, int max_towers, int height_axis,
                       const double* voxel_size_host, const double* center_host, int apply_filter, double threshold,
                       double tower_height, double rim_sq, double min_euc, uint8_t* keep, double* planar, double* agg,
                       int32_t* n_agg, int32_t* status, sn_stream_t stream);

/* replaces: the matching loop of compute_euc_dists (utils/observer_utils.py:413-473, the loop at :456-463): for every
 *           ground-truth tower the nearest proposed tower and their planar distance, plus running totals over tiles.
 * agg [B, max_rows_pred, 2] f64, n_agg [B] i32, status_pred [B] i32: what sn_tower_centroids left for the prediction.
 * gt_stats [B, max_towers_gt, SN_TOWER_NSTAT] i64, gt_n_towers [B] i32: sn_tower_proposals' rows of the ground truth.
 * match [B, Kg] i32, dist [B, Kg] f64, gt_planar [B, Kg, 2] f64 (nullable; NaN absent) as defined above.
 * totals i64[SN_TSCORE_NTOTAL] and dist_total f64[1]: both or neither.  hit_dist > 0, +inf allowed.
 * One launch (one workgroup per tile, integer atomics on totals only) and, with totals, a second single-workgroup launch
 * that sums the hits' distances per tile in row order and over the tiles in a fixed shape.  No workgroup waits for another;
 * no allocation, no synchronisation: capturable.
 * SN_ERR_INVALID_ARG: a null required pointer, B <= 0, max_rows_pred or max_towers_gt < 1, height_axis outside 0..2, a
 * voxel size that is not finite and positive, hit_dist not positive (NaN included), a misaligned pointer, only one of totals
 * / dist_total;  SN_ERR_UNSUPPORTED: max_rows_pred or max_towers_gt > SN_TSCORE_MAX_ROWS, B > 65535. */
int sn_tower_match(const double* agg, const int32_t* n_agg, const int32_t* status_pred, int max_rows_pred,
                   const int64_t* gt_stats, const int32_t* gt_n_towers, int max_towers_gt, int B, int height_axis,
                   const double* voxel_size_host, double hit_dist, int32_t* match, double* dist, double* gt_planar,
                   int64_t* totals, double* dist_total, sn_stream_t stream);


/* ------------------------------------------------------------------------- *
 * K13 -- LAS decode: the point records of an uncompressed .las file -> the scan layout of K9, K10 and K12.
 * replaces: las_to_numpy (utils/pcd_processing.py:99-120) behind lp.read(filename) in build_data_samples
 *           (core/datasets/ts40k.py:73-86): laspy's scaled views of X, Y, Z (int32 * scale + offset in fp64),
 *           np.vstack((las.x, las.y, las.z)).transpose() and np.array(las.classification), all on one host core before
 *           the scan can be uploaded.  Here the record bytes go host-to-device as the file holds them.
 *
 * records:  n records of record_length bytes each, on the device, at ANY byte alignment.  All fields little-endian.
 * X, Y, Z:  int32 at bytes 0, 4 and 8 of a record.
 * pts:      [n,3] f64,  pts[i] = (fl(fl((double)X * sx) + ox), fl(fl((double)Y * sy) + oy), fl(fl((double)Z * sz) + oz)):
 *           the conversion is exact, the product and the sum are each rounded once and never contracted -- numpy's
 *           `X * scale + offset`, which is what laspy's scaled view computes.
 * classes:  [n] f64 (nullable).  Point formats 0..5: (double)(byte 15 & 31) -- the synthetic, key-point and withheld bits
 *           are dropped, as las.classification drops them.  Point formats 6..10: (double)(byte 16).
 * hist:     [256] i64 (nullable), ACCUMULATED, not cleared: hist[c] gains the number of records whose class is c.  The
 *           caller zeroes it, so the chunks of one file add up.
 * Bytes of a record beyond those fields are never interpreted.
 * ------------------------------------------------------------------------- */

/* Records per workgroup and pass of the decode kernel (256): host only -- lets a test put its sizes on the seams. */
int sn_las_chunk_records(void);

/* scale, offset: HOST pointers to three doubles each, read during the call only (they travel as kernel arguments: a
 * captured replay keeps those of capture time).  One launch on `stream`: record_length <= 80 stages a workgroup's byte
 * span in LDS with aligned 16-byte loads issued one pass ahead, longer records are read as aligned dwords; neither issues
 * a byte-wide global load.  The kernel may READ, and never writes, the rest of the aligned 16-byte granules that hold the first and the last
 * byte of `records` (such a granule lies in the same page as a valid byte).  Nothing beyond point n - 1 is written; pts
 * and classes are stored 16 bytes at a time wherever the address allows.  The histogram is summed per workgroup in LDS
 * and added with 64-bit integer atomics: it does not depend on scheduling.  No allocation, no synchronisation: capturable.
 * All byte arithmetic is 64-bit: n * record_length may exceed 2^31.
 * SN_ERR_INVALID_ARG: a null records / pts / scale / offset, n <= 0, point_format outside 0..10, record_length below the
 * format's standard length (20, 28, 26, 34, 57, 63, 30, 36, 38, 59, 67 for formats 0..10) or above 65535, a scale or
 * offset that is not finite, pts / classes / hist not 8-byte aligned;  SN_ERR_UNSUPPORTED: n > 2^36.  All checked before
 * the launch. */
int sn_las_decode(const void* records, int64_t n, int point_format, int record_length, const double scale[3],
                  const double offset[3], double* pts, double* classes, int64_t* hist, sn_stream_t stream);


/* ------------------------------------------------------------------------- *
 * K14 -- SemanticKITTI decode: the velodyne and label bytes of B scans -> the pts / labels layout of K1, K9, K10, K12 and
 *        sn_gather_points, with a per-scan class census.
 * replaces: core/datasets/semKITTI.py:388-403 -- SemLaserScan.open_scan / open_label per scan on one host core
 *           (np.fromfile, reshape((-1, 4)), `label & 0xFFFF`, `label >> 16`), the widening to fp64 and an upload per scan.
 * Provenance: the reference imports SemKITTI_API.auxiliary.laserscan.SemLaserScan (semKITTI.py:26) and does not carry it,
 *           so nothing here can be pinned against the reference's own output.  The layout is the published SemanticKITTI
 *           one: .bin is little-endian float32 [n,4] (x, y, z, remission); .label is little-endian uint32 [n] with the
 *           semantic class in the low 16 bits and the instance id in the high 16.  The oracle is numpy on those definitions.
 *
 * scans:       [total,4] f32, the .bin bytes of B scans concatenated, on the device.
 * label_words: [total] u32, the .label bytes concatenated (nullable: points only).
 * offsets:     [B+1] i64 CSR on the device: scan b owns the points offsets[b] .. offsets[b+1]-1.  Empty scans are legal
 *              anywhere, the first and the last included.
 * pts:         [total,3] f64: the exact widening of x, y, z, by the rule of sn_tiles_unpack's f32 rows -- a NaN keeps its
 *              sign and payload and gets the quiet bit (f32 bits 0x7f800001 -> f64 bits 0x7ff8000020000000, which is what
 *              numpy's astype(float64) gives); -0.0 and denormals are carried.
 * remission:   [total] f32 (nullable): a bit copy of column 3.
 * labels:      [total] f64 (nullable iff label_words is null).  sem = w & 0xFFFF.  Without lut labels[i] = (double)sem.
 *              With lut ([n_lut] i32 on the device) labels[i] = (double)lut[sem] when sem < n_lut; otherwise labels[i] =
 *              -1.0 and unmapped[b] gains one (numpy would raise an IndexError there; the device says so with the counter).
 * instance:    [total] i32 (nullable; needs label_words): (int32)(w >> 16).
 * hist:        [B,n_hist] i64 (nullable; needs label_words), ACCUMULATED, not cleared -- the caller zeroes it: hist[b][c]
 *              gains one for every point of scan b whose output class c satisfies 0 <= c < n_hist.  Negative lut values and
 *              the -1 of an unmapped word are simply not counted.
 * bad:         [B] i32 (nullable), WRITTEN: the points of scan b with a non-finite x, y or z (the remission is not looked at).
 * unmapped:    [B] i32 (nullable; needs lut), WRITTEN: the label words of scan b with sem >= n_lut.
 * ------------------------------------------------------------------------- */

/* Points per workgroup and pass of the decode kernel (256): host only -- lets a test put its sizes on the seams. */
int sn_kitti_chunk_points(void);

/* One launch on `stream`, behind one memset node each for bad and unmapped (as sn_tiles_unpack clears bad).  No allocation,
 * no synchronisation: capturable.  Nothing beyond element total - 1 of any output is written.  The grid is capped at 2048
 * workgroups; beyond 2048 * 256 points every workgroup takes a run of CONSECUTIVE chunks (not a grid stride), so the scan
 * its census belongs to changes only where a scan ends.  The census of a workgroup's current scan is summed in LDS and added
 * with 64-bit (hist) and 32-bit (bad, unmapped) integer atomics, non-zero bins only, when the run enters another scan and
 * at its end; there are no float atomics and the result does not depend on scheduling.  A chunk that straddles one or
 * several scan boundaries credits each scan its own points.  The scan of a pass's first point is found from offsets once
 * per workgroup and pass and stepped from there; it stays inside [0, B) whatever offsets holds.  All index arithmetic is
 * 64-bit.
 * Alignment: scans and label_words may sit at any 4-byte alignment; with a 16-byte-aligned scans a point is one 16-byte
 * load.  The label words are read 16 bytes at a time: the kernel may READ, and never writes, the rest of an aligned 16-byte
 * granule that holds a valid word (such a granule lies in the same page as a valid byte).  pts and labels are stored 16
 * bytes at a time wherever the address allows, 8 bytes at either end otherwise.  pts, labels, hist and offsets are 8-byte
 * aligned, the rest 4-byte; no path issues a byte-wide global access.
 * SN_ERR_INVALID_ARG, all checked before the launch: null scans, pts or offsets; total <= 0; B <= 0; labels without
 * label_words or label_words without labels; instance, lut or hist without label_words; n_lut outside 1..65536 with lut;
 * n_hist outside 1..1024 with hist; unmapped without lut; a misaligned pointer.
 * SN_ERR_UNSUPPORTED: total > 2^36 or B > 2^20. */
int sn_kitti_decode(const void* scans, const void* label_words, int64_t total, const int64_t* offsets, int B,
                    const int32_t* lut, int n_lut, double* pts, double* labels, float* remission, int32_t* instance,
                    int64_t* hist, int n_hist, int32_t* bad, int32_t* unmapped, sn_stream_t stream);


/* ------------------------------------------------------------------------- *
 * K15 -- LAS encode: the scan layout of K9, K10 and K12 -> the point records of an uncompressed .las file.  K13's mirror.
 * replaces: what hands a result back in the format it came in.  The reference writes no LAS; with laspy one would copy xyz
 *           and classes to the host (32 B per point), assign them to the scaled dimensions -- np.rint((x - offset) / scale)
 *           per column -- and pack the unaligned 20..38-byte records, all on one host core.  Here the records are made on
 *           the device and go device-to-host as the file will hold them.
 *
 * Served:   the point formats 0, 1, 2, 3, 6, 7 and 8.  The waveform formats 4, 5, 9 and 10 are SN_ERR_UNSUPPORTED: there is
 *           nothing to synthesise a wave packet from.
 * records:  n records of record_length bytes each, on the device, 16-byte aligned (the writer owns the buffer).
 *           record_length lies between the format's standard length (20, 28, 26, 34, -, -, 30, 36, 38) and 80; the bytes
 *           behind the standard length are written as zero.  The field layout is that of the ASPRS LAS 1.4 specification,
 *           tables 7-15; all fields little-endian.
 * X, Y, Z:  int32 at bytes 0, 4 and 8.  X = rint(fl(fl(x - ox) / sx)): the subtraction and the division are each rounded
 *           once and never contracted, the division is a true IEEE fp64 division (never a product with a reciprocal), rint
 *           rounds half to even -- numpy's np.rint((x - offset) / scale), which is what laspy computes when a scaled
 *           dimension is assigned.  A NaN quotient writes 0, a quotient below -2^31 INT32_MIN, a quotient above 2^31 - 1
 *           INT32_MAX (+-inf included); bad[0] then gains one for the POINT, not one per coordinate.
 * classes:  [n] f64 (nullable: class 0).  c is representable iff c == floor(c) and 0 <= c <= 31 (formats 0..3) or
 *           0 <= c <= 255 (formats 6..8); otherwise 0 is written and bad[1] gains one.  Formats 0..3: byte 15 = c, the
 *           synthetic, key-point and withheld bits zero.  Formats 6..8: byte 16 = c and byte 15 = 0.
 * intensity: [n] u16 (nullable: 0), at byte 12.
 * byte 14:  "return 1 of 1": 0x09 for the formats 0..3, 0x11 for 6..8.
 * gps_time: [n] f64 (nullable: 0), a bit copy to byte 20 (formats 1, 3) or byte 22 (formats 6, 7, 8); SN_ERR_INVALID_ARG
 *           when given for the formats 0 or 2.
 * rgb:      [n,3] u16 (nullable: 0), at byte 20 (format 2), 28 (format 3) or 30 (formats 7, 8); SN_ERR_INVALID_ARG when
 *           given for a format without colour.
 * The NIR field of format 8 and every field not named here (scan angle, user data, point source id, the flag bits) are 0.
 * box:      [6] i32 (nullable), UPDATED with atomic min / max: min X, max X, min Y, max Y, min Z, max Z of the integers
 *           written, saturated ones included.  The caller initialises it to INT32_MAX / INT32_MIN pairs.
 * hist:     [256] i64 (nullable), ACCUMULATED: hist[c] gains the number of records written with class c.
 * bad:      [2] i64 (nullable), ACCUMULATED: points with a coordinate that did not fit, classes that were not representable.
 * The caller zeroes hist and bad, so the chunks of one file add up.
 * ------------------------------------------------------------------------- */

/* Records per workgroup and pass of the encode kernel (256): host only -- lets a test put its sizes on the seams. */
int sn_las_encode_chunk_records(void);

/* scale, offset: HOST pointers to three doubles each, read during the call only (they travel as kernel arguments: a
 * captured replay keeps those of capture time).  One launch on `stream`, no allocation, no synchronisation: capturable.
 * A workgroup builds the byte span of 256 records in LDS and stores it as consecutive 16-byte granules (256 records are a
 * multiple of 16 bytes and records is 16-byte aligned, so every span starts on a granule); only the tail of the LAST span,
 * when n * record_length is no multiple of 16, goes out as one 8-, 4-, 2- and 1-byte store each, as its length needs.  No
 * byte-wide global store in the body of a span.  The kernel writes exactly the bytes [0, n * record_length) of records and
 * not one byte outside.  The inputs are at their element type's natural alignment only (pts, classes, gps_time 8 bytes,
 * intensity, rgb 2 bytes) and nothing outside elements 0 .. n - 1 of them is read.  box, hist and bad are reduced per
 * workgroup on chip and flushed once per workgroup with integer atomics: they do not depend on scheduling.  All byte
 * arithmetic is 64-bit: n * record_length may exceed 2^31.
 * SN_ERR_INVALID_ARG: a null pts / records / scale / offset, n <= 0, point_format outside 0..10, record_length below the
 * format's standard length, a scale that is not finite or is zero, an offset that is not finite, gps_time or rgb for a
 * format that has no such field, records not 16-byte aligned, pts / classes / gps_time / hist / bad not 8-byte, box not
 * 4-byte, intensity / rgb not 2-byte aligned;  SN_ERR_UNSUPPORTED: point_format 4, 5, 9 or 10, record_length > 80,
 * n > 2^36.  All checked before the launch, the SN_ERR_INVALID_ARG ones first. */
int sn_las_encode(const double* pts, const double* classes, const uint16_t* intensity, const double* gps_time,
                  const uint16_t* rgb, int64_t n, int point_format, int record_length, const double scale[3],
                  const double offset[3], void* records, int32_t* box, int64_t* hist, int64_t* bad, sn_stream_t stream);


/* ------------------------------------------------------------------------- *
 * K16 -- coloured voxel clouds: the non-zero voxels of B grids as rows (x, y, z, r, g, b), a CSR batch of B clouds.
 * replaces: the data half of plot_voxelgrid (utils/voxelization.py:45-144) and the color_pointcloud behind it
 *           (utils/pcd_processing.py:525-574): a Python loop over grid.nonzero() and an np.where per voxel on the host, after
 *           a .detach().cpu().numpy() of each logged grid (core/lit_modules/lit_model_wrappers.py:222-233).
 *
 * grid:     [B, n0, n1, n2] = [B, Z, X, Y] of `dtype` (SN_F32 | SN_F64 | SN_U8 | SN_OCC8), element-aligned.  A value is read
 *           as fp64 (an f32 widens exactly).
 * rows:     cloud b holds one row per LIVE cell of tile b, in C order of (z, x, y) -- grid.nonzero() order.  The row is
 *           (x, y, z, 255 r, 255 g, 255 b), all fp64.
 *   SN_CLOUD_DENSITY  live iff value != 0 (-0.0 is zero, NaN is not).  c < 0: (r, g, b) = (1 + c, 1 + c, 1), otherwise
 *                     (1, 1 - c, 1 - c); each sum is rounded once, then multiplied by 255.0 and rounded once, never
 *                     contracted.  A NaN cell is written as (255, NaN, NaN) and counted in bad[b][0] (the reference raises
 *                     IndexError on one).  bad[b][1] counts the live cells that are not NaN and whose colour has a channel
 *                     below 0 or above 255 (|c| > 1).
 *   SN_CLOUD_RANGES   lin = numpy.linspace(0, 1, r) and step = (1 / r) / 2, both formed on the host as numpy forms them.
 *                     Live iff value > lin[1] (NaN, negatives and zero drop out).  The colour is row
 *                     argmin_j |(value - lin[j]) - step| of the table (differences in fp64 in exactly this order, the first
 *                     minimum wins), times 255.0.  The table [r,3] f64 is the caller's (the reference: cm.jet(lin)[:, :3]
 *                     with row 0 forced to (1, 1, 1)).  r is in 2..32 and not read in the density mode.  bad[b] = (0, 0).
 * desc:     null: x, y, z are the cell's indices (i1, i2, i0) as doubles -- the reference's form.  Given: desc
 *           [B, SN_DESC_LEN(n1, n2, n0)] is the voxelisation's descriptor and x, y, z are the voxel centres
 *           (e[k] + e[k+1]) * 0.5 from the tile's own edge tables, the sum and the product rounded once each; a cell whose
 *           upper edge on any axis is not finite (a size-mode padding cell) is not live, whatever it holds -- the rule of
 *           sn_gather_points.  (Build-defined: the reference has no such form.)
 * rgb16:    [capacity,3] u16 for the LAS writer (K15), build-defined: clamp(rint(v), 0, 255) * 257 of the row's 255 r,
 *           255 g, 255 b; NaN gives 0.
 * ------------------------------------------------------------------------- */
#define SN_CLOUD_DENSITY 0
#define SN_CLOUD_RANGES 1

/* Cells per workgroup (1024): host only -- lets a test put its sizes on the seams. */
int sn_voxel_cloud_chunk_cells(void);
/* Workspace bytes of sn_voxel_cloud_count / _scatter for B tiles of V = n0 * n1 * n2 cells: 8 * B * (3 * chunks + 1),
 * chunks = ceil(V / sn_voxel_cloud_chunk_cells()).  0 for a shape the entries refuse (B <= 0, V <= 0, B > 65535, V >= 2^31). */
size_t sn_voxel_cloud_ws_bytes(int B, int64_t V);

/* Live-cell counts of every (tile, workgroup) into ws, their exclusive prefixes per tile in place, the CSR offsets [B+1]
 * (the TRUE sizes) and bad [B,2] i64, reduced from per-workgroup slots in a fixed order.  Three launches on `stream`
 * (count, prefix, offsets); every slot is written by exactly one workgroup: no memset, no atomics, no workgroup waits for
 * another.  No allocation, no synchronisation: capturable; results do not depend on scheduling.
 * SN_ERR_INVALID_ARG: a null grid / ws / offsets / bad, B or an extent <= 0, an unknown mode or dtype, r outside 2..32 in
 * the ranges mode, ws_bytes < sn_voxel_cloud_ws_bytes, a misaligned pointer (grid: its element; the others 8 bytes);
 * SN_ERR_UNSUPPORTED: B > 65535 or n0 * n1 * n2 >= 2^31.  All checked before any launch. */
int sn_voxel_cloud_count(const void* grid, int dtype, int B, int n0, int n1, int n2, int mode, int r, const double* desc,
                         void* ws, size_t ws_bytes, int64_t* offsets, int64_t* bad, sn_stream_t stream);

/* Called with the same grid / mode / r / desc and the ws / offsets that sn_voxel_cloud_count left: writes output row
 * offsets[b] + rank of every live cell whose output index is < capacity into rows [capacity,6] f64 (nullable, 16-byte
 * aligned), xyz [capacity,3] f64 (nullable) and rgb16 [capacity,3] u16 (nullable); one of rows and xyz is given.  Rows at
 * or beyond capacity and everything beyond offsets[B] are NOT touched.  table_host: [r,3] f64 on the HOST, read during
 * the call only (it travels in the launch's arguments: a captured replay keeps the one of capture time); null in the
 * density mode.  One launch; no allocation, no synchronisation: capturable.  Vector stores only.
 * SN_ERR_INVALID_ARG: as sn_voxel_cloud_count (bad aside), and a null table_host in the ranges mode, neither rows nor xyz,
 * capacity < 0, rows not 16-byte, xyz not 8-byte, rgb16 not 2-byte aligned;  SN_ERR_UNSUPPORTED: as sn_voxel_cloud_count. */
int sn_voxel_cloud_scatter(const void* grid, int dtype, int B, int n0, int n1, int n2, int mode, int r,
                           const double* table_host, const double* desc, const void* ws, size_t ws_bytes,
                           const int64_t* offsets, int64_t capacity, double* rows, double* xyz, uint16_t* rgb16,
                           sn_stream_t stream);


/* ------------------------------------------------------------------------- *
 * K17 -- thinning: the rows of a CSR batch kept with a probability per tile and group, compacted in scan order.
 * replaces: the two downsamplers of utils/pcd_processing.py -- downsampling (:375-420) and downsampling_relative_height
 *           (:423-474): a Python loop over the points into a dict of lists keyed by voxel_n / voxel_z, then per group
 *           np.random.rand(len(group)) and group[selected <= threshold].
 *
 * batch:    pts [total,3] f64, labels [total] f64 or null, offsets [B+1] i64 -- the ragged CSR layout of K1, with
 *           offsets[0] = 0 and offsets[B] = total (a row that no tile owns is not kept).  Empty tiles are legal.
 * rule:     row j of tile b (j counted from offsets[b]) is kept iff it is binned and u <= thr[b][g], the comparison
 *           taken literally in fp64: a NaN on either side keeps nothing.  thr [B, G] f64 is the caller's, on the DEVICE.
 *   SN_THIN_GROUP_NONE   g = 0, G = 1.  No descriptor is read (desc, nx, ny, nz are ignored) and every row is binned.
 *   SN_THIN_GROUP_Z      g = the row's z index, G = nz
 *   SN_THIN_GROUP_VOXEL  g = the row's flat [z][x][y] index (iz * nx + ix) * ny + iy, G = nx * ny * nz
 *           The binning is K1's, bit for bit (the same device function as sn_voxel_scatter, the rule stated there), with
 *           desc [B, SN_DESC_LEN(nx, ny, nz)] as sn_voxel_prepare and its siblings build it.  A row with a NaN
 *           coordinate or outside the table on ANY axis is not binned: it is not kept and is counted in unbinned [B].
 *           A size-mode descriptor is accepted with the caveat of sn_voxel_desc_sized: the padded table is used as it
 *           stands, so a foreign row above a tile's own last edge lands in the padding cell n_a, takes that cell's
 *           threshold and is NOT counted in unbinned.
 * uniform:  exactly one of u and seed is given (both on the device).
 *   u     [total] f64, indexed like pts.
 *   seed  [1] u64, READ BY THE KERNEL: a captured graph is re-seeded by a one-element copy.  Row j of tile b draws
 *         Philox4x32-10 (10 rounds, multipliers 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85) with
 *         key (seed lo, seed hi) and counter (j lo, j hi, t lo, t hi), t = tile_ids[b] (i64 [B], nullable: t = b), and
 *         u = ((w0 >> 5) * 2^26 + (w1 >> 6)) * 2^-53 of output words 0 and 1: numpy's 53-bit double, in [0, 1).
 *         A tile's rows depend on its seed, id, points and descriptor alone -- not on its place in a batch.
 * output:   the batch's kept rows in scan order (a stable compaction of the packed array, hence of every tile), as 64-bit
 *           patterns (NaN payloads and -0.0 unchanged, as K7 and K9).  offsets_out [B+1] i64: offsets_out[b] = rows kept
 *           in front of packed index offsets[b] -- the thinned batch's CSR offsets, TRUE sizes whatever the capacity.
 *           first [B, G] u64 (nullable): per group the smallest in-tile index j of any BINNED row, kept or not; all ones
 *           for a group no row falls in.  (What orders the groups as the reference's dict does.)
 * ------------------------------------------------------------------------- */
#define SN_THIN_GROUP_NONE 0
#define SN_THIN_GROUP_Z 1
#define SN_THIN_GROUP_VOXEL 2

/* Workspace bytes of sn_thin_count / sn_thin_scatter: 8 * (2 * (chunks + 1) + 32 * chunks), chunks = ceil(total /
 * sn_thin_chunk_points()) -- two prefix rows and two bits per row of the batch.  0 for a shape the entries refuse
 * (total <= 0, B <= 0, total > 2^33, B > 65536). */
size_t sn_thin_ws_bytes(int64_t total, int B);
/* Rows per workgroup (1024): host only -- lets a test put its sizes on the seams. */
int sn_thin_chunk_points(void);

/* The decision of every row as one bit in ws, the kept and the unbinned counts of every workgroup and their exclusive
 * prefixes, offsets_out [B+1] and unbinned [B].  Three launches on `stream` (count, prefix, offsets), in front of them one
 * memset node over `first` when it is given; `first` is then reduced by 64-bit integer atomic min (an integer minimum:
 * independent of scheduling), the only atomics.  Every slot of ws is written by exactly one workgroup.  No allocation,
 * no synchronisation: capturable.
 * SN_ERR_INVALID_ARG: a null pts / offsets / thr / ws / offsets_out / unbinned, total <= 0, B <= 0, an unknown group, both
 * or neither of u and seed, a group other than SN_THIN_GROUP_NONE with a null desc or an extent <= 0, ws_bytes <
 * sn_thin_ws_bytes(total, B), a pointer that is not 8-byte aligned;  SN_ERR_UNSUPPORTED: total > 2^33, B > 65536,
 * edge tables (nx + ny + nz + 3 doubles, and nz more with SN_THIN_GROUP_Z) beyond 64 KiB of LDS, nx * ny * nz >= 2^31.
 * All checked before any launch. */
int sn_thin_count(const double* pts, const int64_t* offsets, int64_t total, int B, int group, const double* desc, int nx,
                  int ny, int nz, const double* thr, const double* u, const uint64_t* seed, const int64_t* tile_ids, void* ws,
                  size_t ws_bytes, int64_t* offsets_out, int64_t* unbinned, uint64_t* first, sn_stream_t stream);

/* Called with the same batch and rule and the ws that sn_thin_count left: writes the kept row of global rank o (tile b's
 * rows start at offsets_out[b]) for every o < capacity -- out_pts [capacity,3], out_labels [capacity] (null iff labels is
 * null), out_src [capacity] i64 (nullable: the row's index in the packed input), out_key [capacity] i32 (nullable: the
 * row's group g).  Rows at or beyond capacity and everything beyond offsets_out[B] are NOT touched.  The decision is read
 * from ws (one bit per row); it is made again -- same function, same bits -- when out_key is wanted with a grouped rule,
 * to find the groups.  One launch; no allocation, no synchronisation: capturable.
 * SN_ERR_INVALID_ARG: as sn_thin_count (offsets_out, unbinned, first aside), and a null out_pts, capacity < 0, out_labels
 * without labels or the reverse, labels / out_pts / out_labels / out_src not 8-byte or out_key not 4-byte aligned;
 * SN_ERR_UNSUPPORTED: as sn_thin_count. */
int sn_thin_scatter(const double* pts, const double* labels, const int64_t* offsets, int64_t total, int B, int group,
                    const double* desc, int nx, int ny, int nz, const double* thr, const double* u, const uint64_t* seed,
                    const int64_t* tile_ids, const void* ws, size_t ws_bytes, int64_t capacity, double* out_pts,
                    double* out_labels, int64_t* out_src, int32_t* out_key, sn_stream_t stream);


/* ------------------------------------------------------------------------- *
 * K18 -- semantic voxel grids and class colours.
 * replaces: classes_on_voxel (utils/voxelization.py:207-241): a pandas DataFrame of (label, z, x, y),
 *           groupby(["z", "x", "y"]).max() and a Python loop over the occupied voxels into np.zeros; and color_pointcloud
 *           (utils/pcd_processing.py:525-574): np.unique(classes) and a Python loop over every point with
 *           class_color[np.where(unique_classes == c)[0][0]] inside it.
 *
 * batch:    the ragged CSR layout of K1 and K17: offsets [B+1] i64 with offsets[0] = 0 and offsets[B] <= total; rows at or
 *           beyond offsets[B] are neither read for a result nor written.  Empty tiles are legal.
 * grid:     [B, nz, nx, ny] f64.  A row is binned by K1's rule, bit for bit (the same device function as sn_voxel_scatter
 *           and sn_thin_count), with desc [B, SN_DESC_LEN(nx, ny, nz)] as sn_voxel_prepare and its siblings build it.  A row
 *           with a NaN coordinate or outside the table on ANY axis takes no part and is counted in unbinned [B].  A
 *           size-mode descriptor is accepted with the caveat of sn_thin_count: the padded table is used as it stands, so a
 *           foreign row above a tile's own last edge lands in the padding cell n_a and is NOT counted in unbinned.
 *             a voxel no binned row falls in                       +0.0 (the reference starts from np.zeros)
 *             a voxel whose binned rows all carry NaN labels       NaN (pandas' groupby.max of an all-NaN group)
 *             any other voxel                                      the largest label that is not NaN, by value, as its
 *                                                                  64-bit pattern (pandas' max skips NaN); +-inf, negatives
 *                                                                  and denormals are ordinary values; of -0.0 and +0.0 in
 *                                                                  one voxel, +0.0 comes out
 *           Binned or not, a row with a NaN label is counted in nan_labels [B].
 * classes:  [total] f64.  A value is VALID iff it is integral and in 0 .. 65535 (LAS classes are bytes, SemanticKITTI's ids
 *           16 bits; -0.0 is class 0).  present [B, SN_CLASS_WORDS] u32: bit c of tile b (bit c & 31 of word c >> 5) is set
 *           iff some row of the tile holds the valid value c.  rank(c) = the set bits of the tile below c: the index of c in
 *           numpy.unique of the tile's valid classes.
 * ------------------------------------------------------------------------- */
#define SN_CLASS_WORDS 2048
#define SN_VOXEL_CLASSES_NO_SKIP 1

/* Rows per workgroup of sn_voxel_classes (1024) and of sn_class_census / sn_class_paint (8192): host only -- they let a
 * test put its sizes on the seams. */
int sn_voxel_classes_chunk_points(void);
int sn_class_chunk_points(void);

/* The class grid of every tile.  Three launches on `stream` and no memset node: one that zeroes the grid and the counters,
 * one pass over the rows that reduces each row's order-preserving 64-bit key into the grid's own cell by integer atomic max (sent only
 * where a plain load of the cell shows less; flags = SN_VOXEL_CLASSES_NO_SKIP sends it always -- same result, for timing),
 * then one pass that decodes the grid in place.  unbinned and nan_labels are integer atomic sums.  Integer maxima and sums:
 * the result does not depend on scheduling.  No allocation, no synchronisation: capturable.
 * SN_ERR_INVALID_ARG: a null pts / labels / offsets / desc / grid / unbinned / nan_labels, total <= 0, B <= 0, an extent
 * <= 0, unknown flags, a pointer that is not 8-byte aligned;  SN_ERR_UNSUPPORTED: total > 2^33, B > 65536, edge tables
 * (nx + ny + nz + 3 doubles) beyond 64 KiB of LDS, nx * ny * nz >= 2^31.  All checked before any launch. */
int sn_voxel_classes(const double* pts, const double* labels, const int64_t* offsets, int64_t total, int B, const double* desc,
                     int nx, int ny, int nz, int flags, double* grid, int64_t* unbinned, int64_t* nan_labels,
                     sn_stream_t stream);

/* present [B, SN_CLASS_WORDS] and bad [B] i64 (the rows of each tile that are not valid: NaN, fractional, negative, above
 * 65535).  Two launches and no memset node (present, bad <- 0; the rows): every workgroup builds the bitmap of its rows in LDS and merges it with 32-bit
 * atomic OR; bad is an integer atomic sum.  No allocation, no synchronisation: capturable.
 * SN_ERR_INVALID_ARG: a null classes / offsets / present / bad, total <= 0, B <= 0, classes / offsets / bad not 8-byte or
 * present not 4-byte aligned;  SN_ERR_UNSUPPORTED: total > 2^33, B > 65536. */
int sn_class_census(const double* classes, const int64_t* offsets, int64_t total, int B, uint32_t* present, int64_t* bad,
                    sn_stream_t stream);

/* Called with the same batch and the `present` that sn_class_census left.  table [T,3] f64 on the DEVICE.
 *   colors [total,3] f64 (nullable): row i = the 64-bit patterns of table[rank(classes[i])]
 *   rgb    [total,3] u16 (nullable): clamp(rint(255 * c), 0, 255) * 257 of that row's channels, the product rounded once
 *          (K16's rule; NaN gives 0).  At least one of colors and rgb is given.
 *   A row whose rank is >= T is counted in short_table [B] i64; it and a row that is not valid get a NaN row in colors and
 *   zeros in rgb (the reference raises IndexError for both).
 *   n_unique [B] i64: the tile's number of valid classes.  unique [B, U_max] f64 (nullable): the first min(n_unique, U_max)
 *   of them in ascending order -- numpy.unique; the rest of the row is NOT touched.
 * Two launches (one workgroup per tile: n_unique, unique, short_table <- 0; then the rows); no allocation, no
 * synchronisation: capturable.
 * SN_ERR_INVALID_ARG: a null classes / offsets / present / table / n_unique / short_table, neither colors nor rgb, total
 * <= 0, B <= 0, T <= 0, unique with U_max <= 0, a misaligned pointer (present 4 bytes, rgb 2, the others 8);
 * SN_ERR_UNSUPPORTED: as sn_class_census. */
int sn_class_paint(const double* classes, const int64_t* offsets, int64_t total, int B, const uint32_t* present,
                   const double* table, int T, double* colors, uint16_t* rgb, double* unique, int U_max, int64_t* n_unique,
                   int64_t* short_table, sn_stream_t stream);

/* -------------------------------------------------------------------------
 * K19 -- scan merge: the predictions of K tiles put back on the whole scan they were cut from, in one pass.
 * replaces: sn_gather_points over the cropped rows followed by crops.merge_to_scan (five torch launches, a scatter_reduce
 *           through floating-point atomics, the crops' src column) -- the last step of "a corridor scan in, a probability
 *           per scan point out".  (Build-defined: the reference has no whole-scan step.)
 *
 *   grid     [B, channels, nz, nx, ny] of `dtype` (SN_F32 | SN_F64): the tiles' predictions
 *   desc     [B, SN_DESC_LEN(nx,ny,nz)]: the voxelisation's descriptor of every tile, n-mode or size-mode
 *   pts      [n,3] f64: the scan;  regions [K,4] f64, kinds [K] i32 (nullable: all discs): exactly K9's
 *   tile_of  [K] i32 (nullable): the tile of region k.  Null: tile k, and B == K is required.  A value outside 0..B-1: the
 *            region has no tile and covers nothing (how the empty regions a batch dropped are expressed; device memory,
 *            so no entry is refused).  Two regions may share a tile.
 *   out      [channels, n] of `dtype`;  cover [n] i32 (nullable)
 *
 * Covering.  Region k COVERS point i iff (1) k has a tile, (2) the point is a member of k by K9's test taken literally --
 * the same text with the same roundings, z takes no part, a NaN is a member of nothing, a kinds value other than
 * SN_CROP_DISC / SN_CROP_BOX makes the region empty -- and (3) the point bins inside tile tile_of[k]'s edge table by
 * sn_gather_points' rule: at or below the first edge of an axis (-inf included) is bin 0; above the last edge, +inf or NaN
 * is outside; a size-mode padding cell is outside.  A member that bins outside is NOT covered by that tile: it does not
 * contribute `fill` (sn_gather_points + merge_to_scan let it compete with the value `fill`).
 * cover[i] is the number of covering regions; a point with none gets `fill` in every channel.
 *   SN_MERGE_MAX       per channel the largest covering value; NaN if any covering value is NaN (what
 *                      scatter_reduce(amax) gives: a kernel that reports through NaN outputs must surface).
 *   SN_MERGE_MEAN      the covering values widened to fp64 and added in ascending region index, the sum divided by the count
 *                      with one rounding, the quotient rounded to `dtype`.
 *   SN_MERGE_INTERIOR  every channel from the covering region with the largest DEPTH: the first covering region (ascending
 *                      index) is held, a later one replaces it iff its depth > the held depth, so ties go to the lowest
 *                      index (and a NaN depth neither replaces nor is replaced).  Depth is fp64, every operation rounded
 *                      once, never contracted:
 *                        box (xmin, ymin, xmax, ymax):  min(min(x - xmin, xmax - x), min(y - ymin, ymax - y)), min(a, b) =
 *                                                       a < b ? a : b
 *                        disc (cx, cy, r):              sqrt(R2) - sqrt(s), R2 = fl(r*r), s = fl(fl(dx*dx) + fl(dy*dy)) -- the
 *                                                       very two numbers the membership test compares; both roots correctly
 *                                                       rounded
 *                      Depth follows the REGION's geometry, not the grid's: the grid is built from the members' bounding
 *                      cube, which may end short of the region's rim.
 * One launch; no workspace, no atomics, no memset, no allocation, no synchronisation: capturable, and one thread owns one
 * scan point, so no result depends on scheduling.  regions, kinds, tile_of and desc are device memory: a replay follows
 * their current contents.
 * SN_ERR_INVALID_ARG (before the launch): a null grid / desc / pts / regions / out; n, K, B, channels or an extent <= 0;
 * rule outside 0..2; dtype not F32 / F64; tile_of null with B != K; pts / regions / desc not 8-byte, kinds / tile_of /
 * cover not 4-byte, grid / out not element aligned.  SN_ERR_UNSUPPORTED: n > 2^36, K > 65536, channels > 65535, an edge
 * table above 64 KiB (sn_gather_points' bound).
 * ------------------------------------------------------------------------- */
#define SN_MERGE_MAX      0
#define SN_MERGE_MEAN     1
#define SN_MERGE_INTERIOR 2
int sn_scan_merge(const void* grid, int dtype, int channels, int B, int nx, int ny, int nz, const double* desc,
                  const double* pts, int64_t n, const double* regions, const int32_t* kinds,
                  const int32_t* tile_of, int K, int rule, double fill, void* out, int32_t* cover,
                  sn_stream_t stream);


/* ------------------------------------------------------------------------- *
 * K21 -- nearest neighbours: the k smallest neighbour distances of every point within a radius, on K10's cell grid.
 * replaces: avg_dist_points (utils/pcd_processing.py:477-505: a Python loop over all pairs with np.linalg.norm whose list
 *           of distances is sorted again for every point) -- the reference's only question about the spacing of a cloud;
 *           and is the primitive under the k-distance curve (choosing eps / min_points), point spacing (choosing a voxel
 *           size or a thinning rate) and statistical / radius outlier removal.
 *
 * batch:     pts [total,3] f64 with offsets [B+1] i64 on the DEVICE -- the ragged CSR layout of K1 and K17, offsets[0] = 0
 *            and offsets[B] <= total; B = 1 is a whole scan.  Empty tiles are legal.
 * candidate: for row p of tile b, a row q != p (by row index) OF THE SAME TILE with d2 = (dx*dx + dy*dy) + dz*dz <=
 *            radius*radius in fp64, in exactly this form, each product and sum rounded once and never contracted, the
 *            comparison literal: a row with a NaN or infinite coordinate has no candidates and is nobody's candidate.
 *            With SN_KNN_EXCLUDE_ZERO candidates with d2 == 0 are left out (the reference's `if euc > 0`: duplicates go
 *            with the point itself).
 * outputs, indexed by the row's own index in the packed array (scan order):
 *   d2        [total,k] f64: the k smallest candidate d2, ascending; +inf in the columns beyond the candidates
 *   found     [total] i32: the number of candidates within the radius -- ALL of them, not capped at k
 *   mean_dist [total] f64 (nullable): (sqrt(d2[0]) + sqrt(d2[1]) + ...) / c over the c = min(found, k) finite columns,
 *             added in ascending column order, every operation rounded once (sqrt correctly rounded); NaN where found == 0
 *   index     [total,k] i64 (nullable): the packed row indices of those neighbours, -1 beyond min(found, k)
 *   The k are chosen by the lexicographic order (d2, row index): ties do not depend on the order of rows inside a cell.
 *   A row at or beyond offsets[B] belongs to no tile: found 0, +inf, NaN, -1.
 * Every result is a function of the candidate set alone; nothing depends on scheduling.
 * grid:      K10's, an accelerator only: cubic cells of side mult * radius * (1 + 2^-20) -- derived HERE from radius and the
 *            integer mult >= 1, so no caller can hand in a side that breaks the 27-cell claim -- laid from tile b's own
 *            lo [B,3] f64 (device), dims (dim_x, dim_y, dim_z) host integers shared by all tiles, the cell key tile *
 *            cells_per_tile + local cell (tiles never see each other, whatever coordinates they share), B * dim_x * dim_y
 *            * dim_z <= 2^22.  sn_dbscan_cell_grid computes dims and the side (mult = side / (radius * (1 + 2^-20))) for
 *            an extent and a cell budget.  A point outside its tile's grid is clamped into an edge cell: the result is
 *            exact for ANY finite lo and any dims >= 1; they decide the speed only.  dims (1, 1, 1) is brute force.
 * statistics (sn_knn_tile_stats): stats [B, SN_KNN_NSTAT] f64 per tile = n_valid (rows with found >= 1), n_full (rows
 *            with found >= k), sum and sum of squares (each square rounded once) of mean_dist over the valid rows, and
 *            their max (-inf for a tile without a valid row).  Fixed order: partials per chunk of
 *            sn_knn_chunk_points() consecutive rows of a tile, then one combining pass per tile in chunk order; no
 *            floating-point atomics: two runs on the same input give the same bits.
 * ------------------------------------------------------------------------- */
#define SN_KNN_MAX_K 16
#define SN_KNN_NSTAT 5         /* n_valid, n_full, sum, sum_sq, max */
#define SN_KNN_LAUNCHES 4      /* cells, prefix, scatter, search */
#define SN_KNN_EXCLUDE_ZERO 1  /* flags */

/* Rows per workgroup of the kernels and per partial of the statistics (256): host only -- lets a test put its sizes on
 * the seams. */
int sn_knn_chunk_points(void);

/* Workspace bytes of sn_knn_points over `total` rows in B tiles on a grid of cells_per_tile cells per tile (about 36 B per
 * row, 8 B per cell, 40 B per chunk); 0 for what the entry refuses (total < 1 or >= 2^31, B < 1, cells_per_tile < 1, B *
 * cells_per_tile > 2^22).  sn_knn_tile_stats uses the leading bytes of the same workspace, whatever the grid. */
size_t sn_knn_ws_bytes(int64_t total, int B, int64_t cells_per_tile);

/* The search.  k in 1 .. SN_KNN_MAX_K (kept in registers by kernels built for 1, 4, 8 and 16 columns; a k in between runs
 * the next one and stores its first k columns).  SN_KNN_LAUNCHES launches on `stream`, a launch that zeroes the cell
 * populations in front of them (a kernel, not a memset node); integer atomics only, no allocation, no synchronisation:
 * capturable.  radius, dims and mult travel as kernel arguments; pts, offsets and
 * lo are device memory: a replay follows their current contents.
 * SN_ERR_INVALID_ARG: a null pts / offsets / lo / ws / d2 / found, total <= 0, B <= 0, k < 1, a radius that is not finite
 * or <= 0, a dim or mult < 1, unknown flags, pts / offsets / lo / d2 / mean_dist / index not 8-byte, found not 4-byte, ws
 * not 16-byte aligned, ws_bytes < sn_knn_ws_bytes(total, B, dim_x * dim_y * dim_z);  SN_ERR_UNSUPPORTED: k > SN_KNN_MAX_K,
 * total >= 2^31, more than 2^22 cells, a radius outside 1e-150 .. 1e150, mult * radius not finite.  All checked before any
 * launch. */
int sn_knn_points(const double* pts, const int64_t* offsets, int64_t total, int B, double radius, int k, int flags,
                  const double* lo, int dim_x, int dim_y, int dim_z, int64_t mult, void* ws, size_t ws_bytes, double* d2,
                  int32_t* found, double* mean_dist, int64_t* index, sn_stream_t stream);

/* DIAGNOSTIC entry, no part of the stable interface: the launches first..last (1-based, of SN_KNN_LAUNCHES) of the same
 * call and nothing else; tools/knn_bench.py times the prefixes 1..k through it and takes differences.  Launches left out
 * must have run before on the same workspace. */
int sn_knn_points_launches(const double* pts, const int64_t* offsets, int64_t total, int B, double radius, int k, int flags,
                           const double* lo, int dim_x, int dim_y, int dim_z, int64_t mult, void* ws, size_t ws_bytes,
                           double* d2, int32_t* found, double* mean_dist, int64_t* index, int first, int last,
                           sn_stream_t stream);

/* The statistics above from mean_dist and found as sn_knn_points left them (k: the same k).  Two launches (partials,
 * combine), every slot written by one workgroup; capturable.  ws: the workspace of sn_knn_points, or any 16-byte aligned
 * scratch of sn_knn_ws_bytes(total, B, 1) bytes.
 * SN_ERR_INVALID_ARG: a null pointer, total <= 0, B <= 0, k < 1, a misaligned pointer, a short workspace;
 * SN_ERR_UNSUPPORTED: k > SN_KNN_MAX_K, total >= 2^31, B > 65535. */
int sn_knn_tile_stats(const double* mean_dist, const int32_t* found, const int64_t* offsets, int64_t total, int B, int k,
                      void* ws, size_t ws_bytes, double* stats, sn_stream_t stream);


/* ------------------------------------------------------------------------- *
 * K22 -- the shape of a point's neighbourhood: covariance, eigenvalues, normal, principal axis and eigenfeatures of every
 * point's neighbours within a radius, on K10's cell grid.
 * replaces: nothing in the reference (unit_vector / angle_between in utils/pcd_processing.py only orient crops).  This is
 *           THIS project's definition of what every point-cloud toolbox offers per point; ground is planar, a conductor
 *           linear and horizontal, a tower linear and upright, vegetation scattered.
 *
 * batch:     K21's: pts [total,3] f64 with offsets [B+1] i64 on the DEVICE, offsets[0] = 0 and offsets[B] <= total; tiles
 *            never see each other; empty tiles are legal.
 * candidate: K21's test: a row q of the same tile with d2 = (dx*dx + dy*dy) + dz*dz <= radius*radius in fp64, in exactly
 *            this form, each product and sum rounded once and never contracted, the comparison literal: a row with a NaN
 *            or infinite coordinate has no neighbours and is nobody's neighbour.
 * grid:      K21's, an accelerator only: cubic cells of side mult * radius * (1 + 2^-20), derived HERE from radius and the
 *            integer mult >= 1, laid from tile b's own lo [B,3] f64 (device), dims host integers shared by all tiles, B *
 *            dim_x * dim_y * dim_z <= 2^22 (sn_dbscan_cell_grid).  The result is exact for ANY finite lo and any dims >= 1.
 * neighbourhood of row p: p itself and every candidate q != p -- all of them, no cap, duplicates included.
 * count:     found + 1 for a live row that passes its own test (d2 = 0: every finite coordinate), 0 otherwise.
 * moments, in fixed point: with inv = 65536.0 / radius (host, one rounding, a kernel argument) every member contributes
 *            f_a = (int64) rint(fl(q_a - p_a) * inv) for a in {x, y, z}: the difference and the product rounded once each,
 *            rint rounds half to even.  |fl(q_a - p_a)| <= radius (1 + 2^-51) (a member has fl(d_a*d_a) <= fl(radius*radius),
 *            both normal), so |f_a| <= 65537 and f_a is an int32.  The nine moments are int64 sums: S1[3] = sum f_a and
 *            S2[6] = sum f_a * f_b in the order xx, xy, xz, yy, yz, zz.  Integer sums are exact and order-independent: two
 *            runs, any grid and any permutation of the rows give the same bits.  total <= 2^30 is required: a neighbourhood
 *            has at most 2^30 members, |f_a * f_b| <= 65537^2 < 2^32 + 2^18, so |S2| < 2^30 * (2^32 + 2^18) < 2^63 and
 *            |S1| < 2^47: no sum leaves int64.
 * covariance, fp64, every operation rounded once, never contracted (int64 -> fp64 conversions round to nearest even):
 *            n = (double)count, m_a = (double)S1_a / n, C_ab = (double)S2_ab / n - m_a * m_b: the population covariance in
 *            fixed-point units squared (one unit = radius / 65536).  Cancellation: both terms are at most R2 = 65537^2 <
 *            2^32.001 in magnitude and carry at most two roundings each (conversion and quotient; quotient and product), the
 *            difference one more, so |C_ab - exact| <= 5 * 2^-53 * R2 < 2^-18.6 units squared whatever the neighbourhood.
 *            Offsets are measured from p, a member, so they are at most one radius, not a UTM coordinate; a
 *            neighbourhood that spreads one unit or more along an axis has a variance of at least (1/n)(1 - 1/n) units squared
 *            there.  In coordinate units the bound is 2^-18.6 * (radius / 65536)^2 = radius^2 * 2^-50.6.
 * eigen-decomposition: cyclic Jacobi on the symmetric 3x3 A = C with V = I, SN_SHAPE_SWEEPS sweeps, all executed, each the
 *            pairs (p, q) = (0,1), (0,2), (1,2) in this order.  A rotation whose a_pq is exactly 0 is skipped (the only
 *            data-dependent step); otherwise, with r the third index, in + - * / and sqrt only:
 *              theta = (a_qq - a_pp) / (2 * a_pq)
 *              u     = 1 / (|theta| + sqrt(theta * theta + 1))      theta * theta may be +inf: u = 0 and t = +-0
 *              t     = theta < 0 ? -u : u
 *              c     = 1 / sqrt(t * t + 1),  s = t * c,  h = t * a_pq
 *              a_pp' = a_pp - h,  a_qq' = a_qq + h,  a_pq' = 0
 *              a_rp' = c * a_rp - s * a_rq,  a_rq' = s * a_rp + c * a_rq
 *              v_kp' = c * v_kp - s * v_kq,  v_kq' = s * v_kp + c * v_kq     for k = 0, 1, 2
 *            The eigenvalues are the diagonal, the eigenvector of a_jj column j of V.  They are sorted ascending by the
 *            compare-and-swap network (0,1), (1,2), (0,1), a swap only where the left value is GREATER (equal values keep
 *            their index order), the columns carried along.  A vector is then divided by sqrt((x*x + y*y) + z*z) and
 *            negated as a whole where z < 0, or z == 0 and y < 0, or z == y == 0 and x < 0.
 * outputs, indexed by the row's own index in the packed array, each nullable except count:
 *   count   [total] i32
 *   moments [total,9] i64: S1 then S2 -- the raw result of the walk
 *   eig     [total,3] f64: l0 <= l1 <= l2 in squared coordinate units, each lambda_fix * unit2 with unit = radius / 65536.0
 *           (exact) and unit2 = unit * unit (one rounding)
 *   normal  [total,3] f64: the unit eigenvector of l0 under the sign rule;  axis [total,3] f64: that of l2
 *   feat    [total,SN_SHAPE_NFEAT] f64 from the stored eig with negative values clamped to 0 (c0, c1, c2), normal and axis:
 *           linearity (c2 - c1) / c2, planarity (c1 - c0) / c2, scattering c0 / c2, surface variation c0 / ((c0 + c1) + c2),
 *           verticality 1 - |normal_z|, uprightness |axis_z|
 *   A row with count < min_points (an argument >= 3: a plane needs three points) or whose largest fixed-point eigenvalue is
 *   not > 0 (every member coincides with it) has NaN in eig, normal, axis and feat.  A row at or beyond offsets[B] has
 *   count 0, zero moments and NaN in the rest.
 * ------------------------------------------------------------------------- */
#define SN_SHAPE_SWEEPS 4      /* Jacobi sweeps, all executed; chosen on the host: tests/shape_cases.py */
#define SN_SHAPE_NFEAT 6       /* linearity, planarity, scattering, surface variation, verticality, uprightness */
#define SN_SHAPE_LAUNCHES 5    /* zero, cells, prefix, scatter, shape */

/* Rows per workgroup of the kernels (256): host only -- lets a test put its sizes on the seams. */
int sn_shape_chunk_points(void);

/* Workspace bytes of sn_shape_points over `total` rows in B tiles on a grid of cells_per_tile cells per tile (about 36 B
 * per row, 8 B per cell); 0 for what the entry refuses (total < 1 or > 2^30, B < 1, cells_per_tile < 1, B * cells_per_tile >
 * 2^22). */
size_t sn_shape_ws_bytes(int64_t total, int B, int64_t cells_per_tile);

/* SN_SHAPE_LAUNCHES launches on `stream`, all named shape_*; integer atomics only, no allocation, no synchronisation:
 * capturable.  radius, min_points, dims and mult travel as kernel arguments; pts, offsets and lo are device memory: a replay
 * follows their current contents.  flags: none are defined, pass 0.
 * SN_ERR_INVALID_ARG: a null pts / offsets / lo / ws / count, total <= 0, B <= 0, min_points < 3, a radius that is not
 * finite or <= 0, a dim or mult < 1, flags != 0, pts / offsets / lo / moments / eig / normal / axis / feat not 8-byte, count
 * not 4-byte, ws not 16-byte aligned, ws_bytes < sn_shape_ws_bytes(total, B, dim_x * dim_y * dim_z);  SN_ERR_UNSUPPORTED:
 * total > 2^30, more than 2^22 cells, a radius outside 1e-150 .. 1e150, mult * radius not finite.  All checked before any
 * launch. */
int sn_shape_points(const double* pts, const int64_t* offsets, int64_t total, int B, double radius, int min_points,
                    int flags, const double* lo, int dim_x, int dim_y, int dim_z, int64_t mult, void* ws, size_t ws_bytes,
                    int32_t* count, int64_t* moments, double* eig, double* normal, double* axis, double* feat,
                    sn_stream_t stream);

/* DIAGNOSTIC entry, no part of the stable interface: the launches first..last (1-based, of SN_SHAPE_LAUNCHES) of the same
 * call and nothing else; tools/shape_bench.py times the prefixes through it and takes differences.  Launches left out must
 * have run before on the same workspace. */
int sn_shape_points_launches(const double* pts, const int64_t* offsets, int64_t total, int B, double radius, int min_points,
                             int flags, const double* lo, int dim_x, int dim_y, int dim_z, int64_t mult, void* ws,
                             size_t ws_bytes, int32_t* count, int64_t* moments, double* eig, double* normal, double* axis,
                             double* feat, int first, int last, sn_stream_t stream);


/* ------------------------------------------------------------------------- *
 * K23 -- point clouds to images: a point rasteriser with a z-buffer.
 * replaces: nothing the reference computes.  Its visualize_ply, plot_voxelgrid(plot=True), visualize_pred_vs_gt,
 *           plot_centroids and visualize_batch end in a viewer window or a matplotlib 3-D scatter on the host.  This is THIS
 *           project's definition of an image of a point cloud: K16's, K18's and K22's coloured rows (xyz + 16-bit RGB)
 *           become K images of H x W pixels without leaving the device.
 *
 * batch:  the ragged CSR layout of K1, K17 and K18: pts [total,3] f64, offsets [B+1] i64 on the DEVICE with offsets[0] = 0
 *         and offsets[B] <= total; rows at or beyond offsets[B] are neither read nor written.  Empty tiles are legal.
 * views:  K of them, 1 <= K <= SN_RENDER_MAX_VIEWS, all of H x W pixels.  view_tile [K] i32 (device): view k shows tile
 *         view_tile[k]; any order; a tile may have no view or several; a value outside 0 .. B-1 shows nothing.
 *         cam [K,16] f64 (device):  cam[0..11] a 3 x 4 row-major matrix A;  cam[12] kind, 0 orthographic or 1 perspective;
 *         cam[13] near;  cam[14] far;  cam[15] the point size s in pixels, integral, 1 .. SN_RENDER_MAX_SPLAT.
 *         A camera row with an unknown kind, a non-integral or out-of-range s, !(near < far), far - near not finite, or
 *         perspective with near <= 0 shows nothing: its image stays as it was (background after a clearing call) and
 *         bad_views[k] is set to 1.  Checked on the device, where the cameras live.
 * rule:   for row j of tile b (j its index in the tile) and every view k with view_tile[k] == b, literally:
 *
 *           c_r = ((A[r,0]*x + A[r,1]*y) + A[r,2]*z) + A[r,3]        r = 0, 1, 2   (fp64, every operation rounded once)
 *           orthographic:  px = c_0, py = c_1, d = c_2
 *           perspective:   d = c_2;  px = c_0 / d, py = c_1 / d       (true fp64 divisions)
 *           accepted iff   near <= d < far  and  |px| < 2^30 and |py| < 2^30      (NaN anywhere rejects)
 *           dq  = min((u64)floor(((d - near) / (far - near)) * 4294967296.0), 2^32 - 1)
 *           ix  = (i64)floor(px), iy = (i64)floor(py)
 *           key = (dq << 32) | j
 *           for every pixel (X, Y) with ix - (s-1)/2 <= X <= ix + s/2, iy - (s-1)/2 <= Y <= iy + s/2   (integer division)
 *               and 0 <= X < W, 0 <= Y < H:        keys[k, Y, X] = min(keys[k, Y, X], key)      (unsigned 64-bit)
 *           if 0 <= ix < W and 0 <= iy < H:        count[k, iy, ix] += 1                         (count nullable, u32)
 *
 *         Nearest depth wins; among equal depth quanta the lowest row wins.  Integer minima and sums: the result does not
 *         depend on scheduling.  Background is the key of all ones; a tile of 2^32 - 1 rows or more is refused on the
 *         device (nothing of it is drawn and bad_views of its views is set), so no row can produce that key.
 * pixels: a pixel of view k is FOREGROUND iff its key is not all ones, view_tile[k] is in 0 .. B-1 and the key's low word j
 *         is below that tile's number of rows (always so for keys sn_render_splat left with the same batch and views);
 *         every other pixel is background.  The winner is row offsets[view_tile[k]] + j of the packed batch.
 * ------------------------------------------------------------------------- */
#define SN_RENDER_MAX_VIEWS 64
#define SN_RENDER_MAX_SPLAT 9
#define SN_RENDER_ACCUMULATE 1   /* flags: composite onto what keys / count / bad_views hold */
#define SN_RENDER_NO_LOOK 2      /* flags: send every atomic without looking at the pixel first (same result; for timing) */
#define SN_RENDER_LOOK_ALWAYS 4  /* flags: look at the pixel first at every point size, 1 included (same result; for timing) */
#define SN_RENDER_RGB16 0        /* mode: the high bytes of the winner's rgb16 row */
#define SN_RENDER_DEPTH 1        /* mode: the grey 255 - (dq >> 24) */

/* Rows per workgroup of sn_render_splat (256): host only -- lets a test put its tile sizes on the seams. */
int sn_render_chunk_points(void);

/* keys [K,H,W] u64, count [K,H,W] u32 (nullable), bad_views [K] i32.  Without SN_RENDER_ACCUMULATE in `flags` one kernel
 * (no memset node) first sets keys to all ones and zeroes count and bad_views; with it the call composites onto what the
 * three hold -- how a second layer (tower centroids as 9-pixel splats) goes over a scan.  Then ONE pass over the rows: one
 * thread owns one row, reads it once and walks the views of its tile; the rows a workgroup works on at a time belong to one
 * tile, so the view tests are uniform.  Each pixel of a splat of s >= 2 is looked at with a relaxed agent-scope load, and the
 * 64-bit atomic min is sent only where the look shows more than the row's key; at s = 1 the atomic is sent without a look,
 * which measured faster (SN_RENDER_NO_LOOK never looks, SN_RENDER_LOOK_ALWAYS always does; the result is the same).  Vector
 * stores and integer atomics only; no allocation, no synchronisation: capturable.  cam, view_tile, offsets and pts are device
 * memory: a replay follows their current contents.
 * SN_ERR_INVALID_ARG: a null pts / offsets / cam / view_tile / keys / bad_views, total, B, K, H or W <= 0, unknown flags or
 * both look flags, pts / offsets / cam / keys not 8-byte or view_tile / count / bad_views not 4-byte aligned;  SN_ERR_UNSUPPORTED: K >
 * SN_RENDER_MAX_VIEWS, H * W >= 2^31, total > 2^33, B > 65536.  All checked before any launch. */
int sn_render_splat(const double* pts, const int64_t* offsets, int64_t total, int B, const double* cam,
                    const int32_t* view_tile, int K, int H, int W, int flags, uint64_t* keys, uint32_t* count,
                    int32_t* bad_views, sn_stream_t stream);

/* keys -> pixels: one launch, one thread per pixel.  offsets and view_tile are the splat's.
 *   rgba    [K,H,W,4] u8: a foreground pixel takes, in SN_RENDER_RGB16 mode, the HIGH byte of each channel of the winner's
 *           row of rgb16 [total,3] u16 (the inverse of K16's and K18's `* 257`), in SN_RENDER_DEPTH mode the grey
 *           255 - (dq >> 24) (rgb16 may be null); alpha is 255.  A background pixel takes the four bytes of `background`
 *           (r in the low byte, then g, b, a).
 *   index   [K,H,W] i64 (nullable): the winner's row in the packed batch, -1 for background -- the pick buffer.
 *   depth_q [K,H,W] u32 (nullable): dq; 2^32 - 1 for background.
 *   edl     f64, finite and >= 0; 0 turns shading off.  For a foreground pixel o = the sum over its up / down / left / right
 *           neighbours inside the image of max(0, dq_c - dq_n) as a 64-bit integer, dq_n the high word of the neighbour's
 *           key whatever it is (2^32 - 1 for a background neighbour, which so contributes nothing);
 *           shade = 1.0 / (1.0 + edl * ((double)o / 4294967296.0)) and every colour channel c becomes
 *           (u8)floor(c * shade + 0.5), the products, sums and quotients rounded once each.  A pixel with nearer neighbours
 *           is darkened.  No transcendental: numpy gives the same bits.
 * No allocation, no synchronisation: capturable.
 * SN_ERR_INVALID_ARG: a null keys / offsets / view_tile / rgba, B, K, H or W <= 0, an unknown mode, SN_RENDER_RGB16 without
 * rgb16, edl < 0, NaN or infinite, keys / offsets / index not 8-byte, view_tile / depth_q / rgba not 4-byte or rgb16 not
 * 2-byte aligned;  SN_ERR_UNSUPPORTED: K > SN_RENDER_MAX_VIEWS, H * W >= 2^31, B > 65536. */
int sn_render_resolve(const uint64_t* keys, int K, int H, int W, const int64_t* offsets, int B, const int32_t* view_tile,
                      const uint16_t* rgb16, int mode, uint32_t background, double edl, uint8_t* rgba, int64_t* index,
                      uint32_t* depth_q, sn_stream_t stream);


/* ------------------------------------------------------------------------- *
 * K24 -- voxel pooling: per voxel the mean, minimum or maximum of a coordinate or of a per-point value column, in up to
 *        eight planes, and the count of the rows that took part.
 * replaces: Vox.centroid_hist_on_voxel / Vox.centroid_reg_on_voxel, which core/datasets/torch_transforms.py:161-162 calls and
 *           the reference's tree does not contain (build-defined: the mean position of each voxel's points next to the
 *           density and the ratio); and the torch formulation (searchsorted for the flat indices, index_add_ /
 *           scatter_reduce through floating-point atomics, whose sums depend on the order of arrival).
 *
 * batch:    the ragged CSR layout of K1, K17 and K18: pts [total,3] f64, offsets [B+1] i64 with offsets[0] = 0 and
 *           offsets[B] <= total; rows at or beyond offsets[B] are not read.  Empty tiles are legal.
 *           values [total,C] f64 row-major, 0 <= C <= SN_POOL_MAX_COLUMNS; nullable when no plane reads a column.
 * planes:   1 <= P <= SN_POOL_MAX_PLANES.  Plane p reads source plane_source_host[p] (0, 1, 2: x, y, z; 3 + c: value column
 *           c) and reduces with plane_op_host[p] (SN_POOL_MEAN / SN_POOL_MIN / SN_POOL_MAX).  A source may appear in several
 *           planes.  Both lists are HOST arrays read by the call.
 * rows:     a row is binned by K1's rule, bit for bit (the same device function as sn_voxel_scatter, sn_thin_count and
 *           sn_voxel_classes), with desc [B, SN_DESC_LEN(nx, ny, nz)] as sn_voxel_prepare and its siblings build it.
 *             a row with a NaN coordinate or outside the table on ANY axis      counted in unbinned [B] and nowhere else
 *             a binned row with a NaN in a value column that SOME plane reads   counted in nan_rows [B] and nowhere else
 *             every other row                                                   counts 1 in counts [B,nz,nx,ny] i32 and
 *                                                                               takes part in EVERY plane
 *           counts[b].sum() + unbinned[b] + nan_rows[b] == the tile's rows; with no plane on a value column counts equals
 *           sn_voxel_scatter's counts bit for bit.  A size-mode descriptor is accepted with the caveat of sn_thin_count and
 *           sn_voxel_classes: the padded table is used as it stands, so a foreign row above a tile's own last edge lands in
 *           the padding cell n_a and is NOT counted in unbinned.
 * MEAN:     a fixed-point mean, so that the bits depend neither on scheduling nor on the order of the rows.  For a
 *           coordinate source a: lo = desc[b][a], hi = desc[b][3 + a]; for a value source c: lo, hi =
 *           value_range_host[c][0], [1] (HOST, [C,2]; finite with hi > lo for every column a MEAN plane reads; nullable
 *           when none does).  span = fl(hi - lo); inv = fl(4294967296.0 / span) if span > 0 and the quotient is finite,
 *           else 0 (a one-point tile has hi == lo: its centroid is lo).  Per row t = fl(fl(p - lo) * inv); t = t > 0 ? t : 0
 *           (so a NaN product -- an infinite difference times inv = 0 -- is 0); t = t < 2^32 ? t : 2^32; q = (int64)
 *           rint(t).  -inf, -1e300 and every foreign row K1 clips into bin 0 so count as lo, +-inf values as the ends of
 *           their range.  S = the sum of the q by 64-bit integer atomic add; the plane holds fl(lo + fl(fl((double)S /
 *           (double)n) * step)), step = fl(span / 4294967296.0), n the voxel's count, every operation rounded once
 *           (-ffp-contract=off).  Within span * 2^-33 of the fp64 mean of the clamped inputs (half a quantum per row).
 * MIN/MAX:  by value, through the order-preserving 64-bit key of K18 and integer atomic min / max, the plane the winner's
 *           64-bit pattern.  +-inf and denormals are ordinary values; of -0.0 and +0.0 in one voxel MAX gives +0.0 and MIN
 *           -0.0.  (NaN cannot arrive: such a row is in nan_rows.)
 * empty:    a voxel with counts == 0 holds `fill` in every plane, its bit pattern as given.
 * out:      [B, P, nz, nx, ny] f64.
 * ------------------------------------------------------------------------- */
#define SN_POOL_MEAN 0
#define SN_POOL_MIN 1
#define SN_POOL_MAX 2
#define SN_POOL_MAX_PLANES 8
#define SN_POOL_MAX_COLUMNS 5
#define SN_VOXEL_POOL_NO_LOOK 1

/* Rows per workgroup of sn_voxel_pool (1024): host only -- lets a test put its sizes on the seams. */
int sn_voxel_pool_chunk_points(void);
/* Workspace bytes of sn_voxel_pool: 0 for every shape -- the call accumulates in `out` and `counts` themselves, and its `ws`
 * is ignored (null is fine).  Kept in the interface so that a caller sizes a workspace by asking, not by knowing. */
int64_t sn_voxel_pool_ws_bytes(int B, int nx, int ny, int nz, int P);

/* Three launches on `stream` and no memset node: clear (the accumulators to what each reduction starts from, unbinned and
 * nan_rows to 0), rows (per row that takes part one integer atomic add for the count and one 64-bit integer atomic per
 * plane; a min / max atomic is sent only where a plain load of the cell shows that it can still change the cell --
 * flags = SN_VOXEL_POOL_NO_LOOK sends it always: same result, for timing), decode.  Integer sums, minima and maxima: the
 * result does not depend on scheduling.  No allocation, no synchronisation: capturable.
 * The accumulators live in `out` and `counts` themselves (a row's P + 1 atomics go to P + 1 lines 8 * V bytes apart) and
 * decode rewrites `out` in place.  [measured] a workspace of P + 1 consecutive words per voxel was 1.07 - 1.13 times slower
 * on 32 tiles of 10^5 points at 64^3 and was taken out.
 * SN_ERR_INVALID_ARG: a null pts / offsets / desc / out / counts / unbinned / nan_rows / plane list, values null with a plane
 * that reads a column, C or P out of range, a source >= 3 + C, an unknown op, unknown flags, a MEAN plane on a column whose
 * range is missing, not finite or without hi > lo, total <= 0, B <= 0, an extent <= 0, a pointer that is not 8-byte aligned
 * (counts: 4-byte);  SN_ERR_UNSUPPORTED: total >=
 * 2^31 (so that a count fits int32 and a sum int64), B > 65536, nx * ny * nz >= 2^31, edge tables (nx + ny + nz + 3
 * doubles) beyond 64 KiB of LDS.  All checked before any launch; each leaves its message in sn_last_error(). */
int sn_voxel_pool(const double* pts, const double* values, int C, const int64_t* offsets, int64_t total, int B,
                  const double* desc, int nx, int ny, int nz, const int32_t* plane_source_host, const int32_t* plane_op_host,
                  int P, const double* value_range_host, double fill, int flags, void* ws, double* out,
                  int32_t* counts, int64_t* unbinned, int64_t* nan_rows, sn_stream_t stream);


#ifdef __cplusplus
}
#endif
#endif /* SCENENET_HIP_H */
