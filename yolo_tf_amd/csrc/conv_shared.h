// Declarations shared by the convolution translation units (conv_route.hip, conv_igemm.hip, conv_pp.hip, conv_s4.hip, conv_d1.hip, conv_c32.hip, conv_c64.hip,
// conv_wgrad.hip, conv_wgrad3.hip, conv_wgrad_c32.hip) and the epilogue they share (conv_epilogue.h).
#pragma once
#include "common.h"

#define Y2_OOB 0x80000000u   // any offset >= num_records makes the buffer DMA return zeros

// Stream-K hand-off flags (conv_igemm.hip owns the pool): one set = Y2_STREAM_FLAG_WORDS flag words -- one per workgroup -- followed by a
// status block: word [WORDS] counts waits that gave up, word [WORDS + 1] is the wait limit in wall-clock ticks (100 MHz; 0 = default).
#define Y2_STREAM_FLAG_WORDS 1024
#define Y2_STREAM_FLAG_STRIDE (Y2_STREAM_FLAG_WORDS + 64)
#define Y2_SK_DEFAULT_WAIT_TICKS 200000000u      // 2 s: five orders of magnitude above the longest legitimate wait (a partner's tail segment, < 100 us)
#if defined(__HIP_DEVICE_COMPILE__)
// The owner of a stream-K tile waits for the flag of partner workgroup p (called by ONE lane) and clears it.  The wait is bounded: a partition
// bug (a workgroup without work never raises its flag -- the hang behind y2_conv_route's grid clamp) or a lost partner must surface as an error,
// not as a hung device.  On a time-out the launch's results are wrong by construction (the owner sums an unfinished slot, and the late partner's
// flag may be consumed by a later launch of the same flag set): the status word makes yolo2_check_async_errors() return YOLO2_E_LAUNCH and re-zero
// the pool; hosts bound the exposure by polling it every step without a synchronisation (yolo2_async_error_snapshot: TrainSession.step,
// DetectSession.detect) and before anything is written to disk.  The fast path (flag already up) costs one load, as before.
__device__ __forceinline__ void y2_sk_wait_and_clear(unsigned *flags, int p) {
    if (__hip_atomic_load(flags + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u) {
        const unsigned cfg = __hip_atomic_load(flags + Y2_STREAM_FLAG_WORDS + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned long long limit = cfg ? cfg : Y2_SK_DEFAULT_WAIT_TICKS, t0 = wall_clock64();
        while (__hip_atomic_load(flags + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u) {
            __builtin_amdgcn_s_sleep(8);
            if (wall_clock64() - t0 > limit) {
                __hip_atomic_fetch_add(flags + Y2_STREAM_FLAG_WORDS, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                break;
            }
        }
    }
    __hip_atomic_store(flags + p, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);     // exactly one consumer per flag
}
#else
__device__ inline void y2_sk_wait_and_clear(unsigned *, int) {}      // (host pass of a __global__ body)
#endif

// Data-gradient launches whose output IS the gradient dA of a batch-normalised producer layer (a = leaky(bn(y))) can reduce that
// layer's BN + leaky backward sums in their epilogue: Y non-NULL selects it.  Per output element dz = dA * leaky'(z),
// xhat = (y - mean) * rstd; the tile adds its columns' sum(dz * xhat) [plane 0] and sum(dz) [plane 1] to the partial rows the
// forward statistics use.  Replaces one full read of dA and y (bn_bwd_reduce_kernel) per layer with a read of y alone, issued while
// the tile is still in LDS.
struct Y2BnBwd {
    const void *Y;      // pre-normalisation output of the producer layer, [M][Nf] (pixel stride = Nf)
    const float *mean, *var, *gamma, *beta;
    float eps, alpha;
    // bits cleared from the partial-row index mask (Y2_BN_PART_ROWS - 1): grids with more (pixel tile, wave row) pairs than rows wrap
    // around R = 256 >> popcount(stat_mask_inv) rows, chosen by the host so that the consumer that finalises the rows in its prologue
    // (yolo2_bn_leaky_fin & co.) reads few of them while same-address atomic adds stay rare (set_stat_rows in conv_route.hip).  0 = all 256 rows.
    int stat_mask_inv;
};

// LDS / tile plan of one conv_igemm_kernel instantiation -- the ONE place its sizes are derived: the kernel takes its constants from here, and
// the host (conv_route.hip, per line of conv_igemm_table.h) counts the partial rows a pixel tile writes from the same struct.
template <typename T, int BM, int BN, int WGN, int NSTAGE, int CH, int NW> struct Y2IgemmPlan {
    static constexpr int VEC = 16 / (int)sizeof(T);
    static constexpr int ROWB = CH * 16;          // bytes per tile row (CH 16-byte chunks)
    static constexpr int RPI = 64 / CH;           // rows per DMA instruction (1 KiB)
    static constexpr int WGM = NW / WGN;          // NW waves per workgroup, arranged WGM x WGN over the output tile
    static constexpr int TM = BM / WGM / 32, TN = BN / WGN / 32;
    static constexpr int B_IT = (BN / RPI + NW - 1) / NW;
    static constexpr int STAGE = (BM + B_IT * NW * RPI) * ROWB, RING = NSTAGE * STAGE;
    // wide-store epilogue: one padded image of WROWS rows x WCPR 16-byte chunks per wave, in the (idle) DMA ring
    static constexpr int WROWS = TM * 32, WROWB = TN * 32 * (int)sizeof(T), WSTRIDE = WROWB + 16, WCPR = WROWB / 16;
    static constexpr int IMAGES = NW * WROWS * WSTRIDE;
    static constexpr bool WIDE_FITS = IMAGES <= RING;      // (K-sliced launches never take it)
    // BN-backward sums: the wave rows of a tile meet in LDS where the ring leaves room behind the images (conv_epilogue.h y2_wave_rows_meet)
    static constexpr bool RED = WGM > 1 && IMAGES + NW * WCPR * 2 * VEC * 4 <= RING;
    // partial rows one pixel tile writes: forward statistics one per wave row; BN-backward sums one where the wave rows meet
    static constexpr int STAT_ROWS_FWD = WGM, STAT_ROWS_BNBWD = RED ? 1 : WGM;
};
// ... of the fixed-tile kernels (256 pixels per tile).  conv_pp.hip: forward one row per wave row, BN-backward one per tile (its wave rows meet in
// LDS); conv_s4.hip: one per 64-row group -- (wave row, half) -- in both forms; conv_d1.hip: one per workgroup, wrapped around D1_STAT_ROWS
constexpr int Y2P_STAT_ROWS_FWD = 4, Y2P_STAT_ROWS_BNBWD = 1;
constexpr int Y2S_STAT_ROWS_FWD = 4, Y2S_STAT_ROWS_BNBWD = 4;
constexpr int D1_STAT_ROWS = 32;

// conv_pp.hip / conv_s4.hip: the tap-fused 3x3 kernels (bf16, 256 x 128 tile) keep a halo image of the input rows in LDS: images up to 55 pixels wide.
// The ONE place that says so: the launch rule asks before it names the family, the two launchers refuse anything else.
inline bool y2_pp_fits(int W) { return W <= 55; }
// conv_pp.hip: ping-pong tap-fused 3x3 kernel; returns non-zero when !y2_pp_fits(W) or `sched` names a schedule this build does not have
int y2_conv3x3_pp_launch(const void *P, unsigned p_bytes, const void *F, unsigned f_bytes, const float *bias, void *O, float *ws, int H, int W, int Cp,
                         int ldp, int Nf, int ldo, int M, int NT, const float *bn_shift, float *bn_part, unsigned *sk_flags, float act_alpha,
                         const Y2BnBwd &bz, int k_rotate, int grid, int sched, int cv, hipStream_t st);

// conv_s4.hip: the loader / consumer member of the same family (four computing waves of 128 x 64, four loader waves); same contract
int y2_conv3x3_s4_launch(const void *P, unsigned p_bytes, const void *F, unsigned f_bytes, const float *bias, void *O, float *ws, int H, int W, int Cp,
                         int ldp, int Nf, int ldo, int M, int NT, const float *bn_shift, float *bn_part, unsigned *sk_flags, float act_alpha,
                         const Y2BnBwd &bz, int k_rotate, int grid, int abl, hipStream_t st);

// conv_wgrad3.hip: 3x3 filter gradient with one kernel row of taps per workgroup over a padded pixel index (bf16).  variant < 0: the shape is not
// taken (conv_wgrad.hip's per-tap kernel runs instead).
struct Y2W3Plan { int variant, ks, qchunk, blocks, remap, direct, BC, BN, waves; };
Y2W3Plan y2_wgrad3_plan(int B, int H, int W, int Cin, int Cout, int cus, int force_variant);
// ws != nullptr (workspace form, a split plan only): the workgroup of pixel range r stores its partial tile into slot r of ws, nothing touches dW
int y2_wgrad3_launch(const Y2W3Plan &p, const void *X, const void *dY, float *dW, int B, int H, int W, int Cin, int ldx, int Cout, int ldy, hipStream_t st,
                     float *ws = nullptr);
// Workspace form of the split filter gradients (yolo2_conv2d_wgrad_ws): floats between two slots of the workspace -- one filter gradient
// [taps][Cin][Cout], rounded up to 16 bytes so that every slot can be read with 16-byte loads
__host__ __device__ inline long y2_wgrad_slot_stride(int taps, int Cin, int Cout) { return ((long)taps * Cin * Cout + 3) & ~3L; }
void y2_magic_u32(unsigned d, unsigned *m, unsigned *s);

// conv_wgrad_c32.hip: 3x3 filter gradient for 32 input channels and 64 filters (Darknet-19 conv1), bf16: all nine taps in one workgroup over a run of image
// rows, every operand byte read once.  y2_w32_wgrad returns non-zero when the rows do not fit its LDS plan (the caller then takes the per-tap kernel).
bool y2_w32_shape(int Cin, int ldx, int Cout, int ldy, int ksize, int dtype);
int y2_w32_blocks(int B, int H, int W, int cus);      // workgroups of the launch; 0: not taken
int y2_w32_wgrad(const void *X, const void *dY, float *dW, int B, int H, int W, int cus, int *blocks, hipStream_t st, float *ws = nullptr);      // ws: one slot per workgroup

// The persistent families size themselves from the shape and the workgroup count alone.  Each has ONE pure geometry function: the launch rule
// (conv_route.hip) and the family's own launcher both call it.  grid == 0: the shape is not taken (it does not fit the kernel's LDS plan, or the form
// that would run has no such epilogue) and the generic kernels run.
struct Y2PersistentPlan { int grid; int rows; size_t lds; };      // workgroups, partial rows the statistics touch (0: none), dynamic LDS bytes

// conv_c32.hip: persistent 3x3 forward for 32-channel inputs and 64 filters (Darknet-19 conv1), bf16.  y2_c32_fwd returns non-zero when the plan does
// not take the shape or the LDS limit cannot be raised (the caller then takes the generic kernels).
bool y2_c32_shape(int Cp, int ldp, int Nf, int ldo, int ksize, int dtype);
struct C32Geo;
Y2PersistentPlan y2_c32_plan(int B, int H, int W, int cus, C32Geo *geo = nullptr);      // (geo: conv_c32.hip's own use)
int y2_c32_fwd(const void *P, const void *F, void *O, int B, int H, int W, const float *bias, float alpha, const float *bn_shift, float *bn_part,
               int cus, hipStream_t st);

// conv_c64.hip: persistent 3x3 convolution for 64-channel inputs with 128 filters (Darknet-19 conv2 / conv4 forward) or 32 (conv1's data gradient), and
// for 128-channel inputs with 64 filters (conv2 / conv4's data gradients), bf16, filters held in registers, one ring of pixel rows per workgroup.
// `epilogue`: bias, activation or statistics are asked for (the 32- and 64-filter forms store plainly and step aside).
bool y2_c64_shape(int Cp, int ldp, int Nf, int ldo, int ksize, int dtype);
struct C64Geo;
Y2PersistentPlan y2_c64_plan(int B, int H, int W, int Nf, bool epilogue, int cus, C64Geo *geo = nullptr);      // (geo: conv_c64.hip's own use)
int y2_c64_fwd(const void *P, const void *F, void *O, int B, int H, int W, int Nf, const float *bias, float alpha, const float *bn_shift, float *bn_part,
               int cus, hipStream_t st);

// conv_d1.hip: persistent 1x1 data gradient + the producer layer's BN / leaky backward sums for the wide early stages (conv3 / conv6), bf16
bool y2_d1_shape(int Cp, int ldp, int Nf, int ldo, int ksize, int dtype, long M);
Y2PersistentPlan y2_d1_plan(long M, int Nf, int cus);      // (grid = workgroups per column group; Nf / 128 groups)
int y2_d1_dgrad_bn(const void *P, const void *F, void *O, long M, int Cp, int Nf, float *bn_part, const Y2BnBwd &bz, int cus, hipStream_t st);

// ---- the generic implicit-GEMM kernels (conv_igemm.hip), as the launch rule (conv_route.hip) sees them ----
struct Y2IgemmKey { int dtype, BM, BN, WGN, stages, KS, split, ctail, chunks, waves, bnbwd; };      // one conv_igemm_kernel instantiation
struct Y2IgemmArgs {      // the kernel's arguments, in its order
    const void *P; unsigned p_bytes; const void *F; unsigned f_bytes; const float *bias; void *O; float *ws; int H, W, Cp, ldp, Nf, ldo, M, NT, remap;
    const float *bn_shift; float *bn_part; unsigned *sk_flags; float act_alpha; int wide_store; Y2BnBwd bz;
};
// A line of conv_igemm_table.h: its launcher, and what the rule reads of its LDS / tile plan (Y2IgemmPlan) -- do the wide-store images fit the ring
// (the BN-backward epilogue reduces from them), the partial rows one pixel tile writes.  y2_igemm_line: nullptr = no such line is built.
struct Y2IgemmLine { Y2IgemmKey key; bool wide_fits; int rows_fwd, rows_bnbwd; void (*launch)(int grid_x, int grid_y, const Y2IgemmArgs &a, hipStream_t st); };
const Y2IgemmLine *y2_igemm_line(const Y2IgemmKey &key);
// K-sliced launches: f32 partial sums [M][Nf] in the workspace -> O (+ bias, activation)
void y2_splitk_finish(const float *acc, const float *bias, void *O, long M, int Nf, int ldo, float act_alpha, int dtype, hipStream_t st);
// the next set of stream-K hand-off flags of the current device (round-robin); NULL: no pool (allocation failed)
unsigned *y2_stream_flags();
int y2_sk_unclamped();      // tests only (yolo2_debug_set_streamk_wait_us): a forced stream-K grid may exceed the number of K steps
