// The launch rule of the forward / data-gradient convolutions, and the yolo2_conv2d* entry points.  Host code only.
//
//   y2_conv_route(call)   PURE: which kernel family and instantiation a call gets, its grid, what else has to be enqueued around it (workspace memset,
//                         finishing kernel, statistics pass) and what the debug queries will report.  No HIP call, no allocation, no global written:
//                         everything the decision reads is a field of Y2ConvCall, the knobs included (a snapshot).
//   y2_conv_launch(route) launches what the route names -- a switch on the family -- and is the only writer of the "last plan" words.  A refusal that
//                         only the runtime can produce (no flag pool, the LDS limit cannot be raised, a schedule this build lacks) comes back as the
//                         Y2X_* bit of the feature that refused; conv2d_impl adds it to the call's exclusions and routes again, so the kernel that
//                         runs is the one the rule gives without that feature.
//   the queries           yolo2_conv2d_workspace_bytes, yolo2_conv2d_dgrad_bn_fuses and yolo2_debug_conv_route are computed from the helpers the
//                         route uses; tests/test_conv_route_cpu.py pins the rule on recorded shapes without a device (tests/golden/conv_plans.json).
// A new kernel is one more case in y2_conv_route and one in y2_conv_launch.
#include "common.h"
#include "conv_shared.h"
#include <algorithm>
#include <atomic>

enum { Y2F_FIRST = 0, Y2F_C32, Y2F_C64, Y2F_D1, Y2F_PP, Y2F_S4, Y2F_IGEMM };                 // family (conv_first / c32 / c64 / d1 / pp / s4 / igemm .hip)
enum { Y2M_PLAIN = 0, Y2M_BIAS_ACT, Y2M_BN_FWD, Y2M_DGRAD_BN };                              // mode: what the call asks of the epilogue
enum { Y2S_NONE = 0, Y2S_EPILOGUE, Y2S_COLSUM, Y2S_TWO_STEP };                               // where the statistics / BN-backward sums come from
enum { Y2X_FIRST = 1, Y2X_C32 = 2, Y2X_C64 = 4, Y2X_D1 = 8, Y2X_PP = 16, Y2X_S4 = 32, Y2X_FLAGS = 64 };      // exclusions (FLAGS: everything stream-K)
enum { Y2A_O16 = 1, Y2A_F16 = 2, Y2A_Y16 = 4 };                                              // 16-byte alignment of O, F and bwd->Y

// ---- knobs (environment, read once per process; debug setters, process-wide) ----
// tap-fused 3x3 variant on/off (default: env YOLO2_IGEMM_TAP, else on); yolo2_debug_set_igemm_tap flips it at run time so that
// tests can compare both variants on the same inputs
// 0 = per-tap kernels only, non-zero = the ping-pong tap-fused kernel (conv_pp.hip) where its launch rule admits it (default).  (The round-2
// tap-fused kernel it replaced -- slower on every layer it took, profiles/r04_pp2_sched_b16.txt column tap-r2 -- is gone.)
// 3 = the loader / consumer member of the tap-fused family (conv_s4.hip: four computing waves of 128 x 64 + four loader waves), same launch rule
static std::atomic<int> g_igemm_tap{y2_env_int("YOLO2_IGEMM_TAP", 2)};
extern "C" int yolo2_debug_set_igemm_tap(int mode) { g_igemm_tap.store(mode == 3 ? 3 : (mode != 0 ? 2 : 0), std::memory_order_relaxed); return YOLO2_OK; }
static std::atomic<int> g_s4_abl{0};      // experiments build of conv_s4.hip: timing ablations / phase stamps (yolo2_debug_set_s4_abl)
extern "C" int yolo2_debug_set_s4_abl(int abl) { g_s4_abl.store(abl, std::memory_order_relaxed); return YOLO2_OK; }
// ping-pong kernel knobs (A/B runs and tests): grid 0 = by rule, 1 = stream-K (one workgroup per CU), 2 = one workgroup per tile;
// dmapos 0/1 = DMA pieces at the head of the LOAD phase / inside the MFMA phase; min_steps, min_share = the launch gates below (< 0: keep)
static std::atomic<int> g_pp_grid{0};
static std::atomic<int> g_pp_dmapos{y2_env_int("YOLO2_PP_SCHED", 2)};      // conv_pp.hip SCHED (2 = fragment reads, then the DMA pieces)
static std::atomic<long> g_pp_min_steps{18};
static std::atomic<long> g_pp_min_share{24};
// cost units charged to the owner of a stream-K tile, in K steps (conv_pp.hip "cost-balanced shares"); 0 = equal K-step shares (round 5).  6 = what
// a second prologue costs a two-segment workgroup: the dominant launches 54.46 -> 53.9 us, the step -12 us, batch 8 / multi-scale equal or better;
// 8 and more lose again -- the owner then waits for partners that take longer (profiles/r06_pp_cv_sweep.txt, its last block)
static std::atomic<int> g_pp_cv{y2_env_int("YOLO2_PP_CV", 6)};
extern "C" int yolo2_debug_set_pp_cost(int cv) {
    if (cv < 0 || cv > 4096) { yolo2_set_error("yolo2_debug_set_pp_cost: 0 .. 4096 K steps"); return YOLO2_E_ARG; }
    g_pp_cv.store(cv, std::memory_order_relaxed); return YOLO2_OK;
}
extern "C" int yolo2_debug_set_pp(int grid, int dmapos, int min_steps, int min_share) {
    if (grid != -1) g_pp_grid.store(grid, std::memory_order_relaxed);
    if (dmapos >= 0) g_pp_dmapos.store(dmapos, std::memory_order_relaxed);
    if (min_steps >= 0) g_pp_min_steps.store(min_steps, std::memory_order_relaxed);
    if (min_share >= 0) g_pp_min_share.store(min_share, std::memory_order_relaxed);
    return YOLO2_OK;
}

// Stream-K launches take exactly one workgroup per CU.  A process that shares the GPU with persistent kernels of another stream -- an
// RCCL ring holds one workgroup per channel for the whole collective -- would get a second, mostly idle wave of workgroups on the CUs
// that are left; yolo2_set_stream_workgroups(n) (data-parallel sessions: CUs - [mi355x] comm_cus) sizes the launches for the CUs that
// are free.  0 restores the default (all CUs, or YOLO2_IGEMM_STREAM_WGS).  Correctness never depends on the value: owners only wait
// for parked tails, and a tail is the first thing its workgroup does (deadlock-free under any residency; tests/test_streamk_occupied_gpu.py).
static std::atomic<int> g_stream_wgs{0};
static int default_stream_wgs() { static const int n = y2_env_int("YOLO2_IGEMM_STREAM_WGS", y2_device_cus()); return n; }
extern "C" int yolo2_set_stream_workgroups(int n) {
    if (n < 0 || n > Y2_STREAM_FLAG_WORDS) { yolo2_set_error("yolo2_set_stream_workgroups: 0 (default) .. %d", Y2_STREAM_FLAG_WORDS); return YOLO2_E_ARG; }
    g_stream_wgs.store(n, std::memory_order_relaxed); return YOLO2_OK;
}
extern "C" int yolo2_get_stream_workgroups(void) { const int n = g_stream_wgs.load(std::memory_order_relaxed); return n > 0 ? n : default_stream_wgs(); }

// what the rule reads of the knobs, taken once per call
// (stream: YOLO2_IGEMM_STREAM=0 -- no stream-K anywhere, for an A/B or debugging a hand-off; first_direct .. d1: YOLO2_FIRST_DIRECT / _C32 / _C64 /
// _D1 = 0 -- the family steps aside; fuse_*: YOLO2_FUSE_BN_BWD, YOLO2_FUSE_BN_BWD_NARROW, see y2_dgrad_bn_fuses)
struct Y2ConvKnobs {
    int tap, s4_abl, pp_grid, pp_sched, pp_cv, pp_long_share, sk_unclamped; long pp_min_steps, pp_min_share;
    bool stream, first_direct, c32, c64, d1, fuse_bn_bwd, fuse_bn_bwd_narrow;
};
static Y2ConvKnobs knobs_now() {
    static const Y2ConvKnobs env{0, 0, 0, 0, 0, y2_env_int("YOLO2_PP_LONG_SHARE", 26) /* (0 = round 4's rule, for the A/B) */, 0, 0, 0, y2_env_int("YOLO2_IGEMM_STREAM", 1) != 0,
                                 y2_env_int("YOLO2_FIRST_DIRECT", 1) != 0, y2_env_int("YOLO2_C32", 1) != 0, y2_env_int("YOLO2_C64", 1) != 0, y2_env_int("YOLO2_D1", 1) != 0,
                                 y2_env_int("YOLO2_FUSE_BN_BWD", 1) != 0, y2_env_int("YOLO2_FUSE_BN_BWD_NARROW", 0) != 0};
    const auto rl = std::memory_order_relaxed;
    Y2ConvKnobs k = env;
    k.tap = g_igemm_tap.load(rl); k.s4_abl = g_s4_abl.load(rl); k.pp_grid = g_pp_grid.load(rl); k.pp_sched = g_pp_dmapos.load(rl); k.pp_cv = g_pp_cv.load(rl);
    k.sk_unclamped = y2_sk_unclamped(); k.pp_min_steps = g_pp_min_steps.load(rl); k.pp_min_share = g_pp_min_share.load(rl);
    return k;
}

// Everything the rule reads.  align: Y2A_* bits; has_ws / ws_bytes: a workspace pointer was given, and its size; cus: workgroups of a one-per-CU
// launch (the device's CUs, or yolo2_set_stream_workgroups / YOLO2_IGEMM_STREAM_WGS); deterministic: the calling thread's mode (no K slicing: its
// slices meet in f32 atomics); exclude: Y2X_* bits, families and features that must not be named
struct Y2ConvCall {
    int B, H, W, Cp, ldp, Nf, ldo, ksize, dtype, mode, align;
    bool has_ws; size_t ws_bytes; int cus; bool deterministic; unsigned exclude; Y2ConvKnobs knobs;
};
// What to launch.  igemm: `ig` names a line of conv_igemm_table.h, `line` is that line (nullptr: none -- an internal error, reported by the launch);
// grid_y: K slices (igemm), column groups (d1); use_ws: the kernel gets the workspace pointer; flags: a set of stream-K hand-off flags is needed;
// memset_ws, finish: K-sliced -- zero the f32 [M][Nf] image first, splitk_finish_kernel afterwards; cv: pp's owner cost; stats: Y2S_*; kernel_stats:
// the kernel gets bn_part; stat_rows: yolo2_last_bn_part_rows (0: the launch writes none and leaves the value); stat_mask_inv: Y2BnBwd's; pending:
// dgrad_bn's *pending; plan: yolo2_debug_last_conv_plan
struct Y2ConvRoute {
    int family; Y2IgemmKey ig; const Y2IgemmLine *line;
    int grid_x, grid_y, NT, remap, wide_store, cv;
    bool use_ws, flags, memset_ws, finish, kernel_stats;
    int stats, stat_rows, stat_mask_inv, pending, plan[8];
};

// number of K slices: when the M x N tile grid alone cannot fill 256 CUs with ~2-3 resident workgroups
// each, slice K so that it does, keeping >= 8 K tiles per slice
static int choose_ksplit(long tiles, int nk) {
    // measured (profiles/): pays for the 88-tile data gradients; elsewhere atomics + the finishing pass cost more than
    // the 8-wave / wide-K variants gain
    if (nk < 128 || tiles > 128) return 1;
    const int ks = (int)((352 + tiles - 1) / tiles), max_ks = nk / 8;      // (352 workgroups: K slicing only for grids below half the chip)
    return ks > max_ks ? max_ks : ks;
}
// one f32 tile slot per workgroup of a stream-K launch
static size_t stream_ws_bytes(int cus, int BM) { return (size_t)cus * BM * 128 * sizeof(float); }

// Partial rows a statistics-producing launch touches (yolo2_last_bn_part_rows): what the consumer's prologue has to sum.  Up to
// Y2_BN_PART_ROWS (pixel tile, wave row) pairs get a row each (plain stores, one writer per element); larger grids wrap around
// R rows with f32 atomic adds, R chosen for <= ~170 adds per address (the 104x104 layer; 20-90 elsewhere) and <= 128 rows to read.
// most rows the consumer's prologue accepts for Nf channels (bn.hip fin_shape_ok: rows x slice x 8 bytes <= 128 KB), <= 256
static void set_stat_rows(Y2ConvRoute &r, long wave_rows, int Nf, int vec) {
    const int lpr = Nf / vec > 16 ? 16 : Nf / vec < 1 ? 1 : Nf / vec;
    const long lim = (128L << 10) / ((long)lpr * vec * 8), limit = lim > Y2_BN_PART_ROWS ? Y2_BN_PART_ROWS : lim;
    int rows = (int)wave_rows;            // one row per (pixel tile, wave row): plain stores
    // (<= ~16 adds per address: same-address f32 atomics serialise at ~0.1 us each -- 42 per address cost the 52 x 52 BN-backward launch 12 us)
    // (batch 8, 26x26 stage: 172 unique rows x 512 channels were more than the consumer reads -- those five layers fell back to the
    // separate finalisation launches; they now wrap around 16 rows like the larger grids)
    if (wave_rows > limit) {
        for (rows = 16; rows < 128 && (long)rows * 16 < wave_rows;) rows <<= 1;
        while (rows > limit) rows >>= 1;
    }
    r.stat_rows = rows;
    r.stat_mask_inv = wave_rows <= limit ? 0 : (Y2_BN_PART_ROWS - 1) ^ (rows - 1);
}

// Does yolo2_conv2d_dgrad_bn take the producer layer's sums from its own epilogue for this shape?  (The answer the rule gives before the variant
// is known: K-sliced variants, channel tails and the f32 rings without a wide-store image still fall back inside the call -- Y2S_TWO_STEP.)
// A/B: YOLO2_FUSE_BN_BWD=0 never; YOLO2_FUSE_BN_BWD_NARROW=1 also the 3x3 data gradients with <= 64 filters on >= 100k pixels -- conv4's at batch 16,
// where the fused epilogue costs the per-tap kernel 32 us and the separate reduction 19: those run plain by default, and a host that asks first
// (yolo2_conv2d_dgrad_bn_fuses) schedules reduction + folded apply itself.
static bool y2_dgrad_bn_fuses(const Y2ConvKnobs &k, int B, int H, int W, int Nf, int ksize, int dtype) {
    return k.fuse_bn_bwd && Nf % (dtype == YOLO2_BF16 ? 8 : 4) == 0 && (k.fuse_bn_bwd_narrow || !(ksize == 3 && Nf <= 64 && (long)B * H * W >= 100000));
}

static Y2ConvRoute y2_conv_route(const Y2ConvCall &c) {
    Y2ConvRoute r{};
    const Y2ConvKnobs &k = c.knobs;
    const int B = c.B, H = c.H, W = c.W, Cp = c.Cp, Nf = c.Nf, ksize = c.ksize, cus = c.cus;
    const bool is_bf16 = c.dtype == YOLO2_BF16, bn = c.mode == Y2M_BN_FWD, bwd = c.mode == Y2M_DGRAD_BN, epilogue = bn || c.mode == Y2M_BIAS_ACT;
    const int VEC = is_bf16 ? 8 : 4;
    const long M = (long)B * H * W;
    r.stats = bn ? Y2S_EPILOGUE : bwd ? Y2S_TWO_STEP : Y2S_NONE; r.kernel_stats = bn; r.grid_y = 1;      // (two-step: until a kernel with the sums in its epilogue is named)
    auto set_plan = [&r](std::initializer_list<int> words) { std::copy(words.begin(), words.end(), r.plan); };
    // a family with a fixed geometry takes the call: its grid, the partial rows its statistics touch (0: none written), its plan words
    auto take = [&](int family, int grid_x, int grid_y, int rows, std::initializer_list<int> words) {
        r.family = family; r.grid_x = grid_x; r.grid_y = grid_y; r.stat_rows = rows; set_plan(words);
        return r;
    };
    if (k.first_direct && !(c.exclude & Y2X_FIRST) && (c.mode == Y2M_PLAIN || bn) && y2_first_layer_shape(Cp, c.ldp, Nf, c.ldo, ksize))      // image layer: direct kernel (conv_first.hip)
        return take(Y2F_FIRST, 0, 1, Y2_BN_PART_ROWS, {-1, -1, -1, -1, -1, -1, -1, -1});
    if (k.c32 && !(c.exclude & Y2X_C32) && !bwd && y2_c32_shape(Cp, c.ldp, Nf, c.ldo, ksize, c.dtype) && (c.align & Y2A_O16)) {      // 32 -> 64 channels (conv1): persistent kernel (conv_c32.hip)
        const Y2PersistentPlan pl = y2_c32_plan(B, H, W, cus);
        if (pl.grid) return take(Y2F_C32, pl.grid, 1, bn ? pl.rows : 0, {512, 64, 8, 8, 9, 0, pl.rows, 1});
    }
    if (k.c64 && !(c.exclude & Y2X_C64) && !bwd && y2_c64_shape(Cp, c.ldp, Nf, c.ldo, ksize, c.dtype) && (c.align & Y2A_O16) && (c.align & Y2A_F16)) {
        // 64 -> 128 channels (conv2 / conv4), 64 -> 32 (conv1's data gradient), 128 -> 64 (conv2 / conv4's data gradients): filters in registers (conv_c64.hip)
        const Y2PersistentPlan pl = y2_c64_plan(B, H, W, Nf, epilogue, cus);
        if (pl.grid) return take(Y2F_C64, pl.grid, 1, bn ? pl.rows : 0, {Nf == 64 ? 128 : 256, Nf, 8, 8, 9, 0, pl.rows, 1});      // (positions per tile, filters)
    }
    // data gradient + the producer layer's BN / leaky backward sums (yolo2_conv2d_dgrad_bn): `bz` -- the kernel is asked for them
    const bool bz = bwd && y2_dgrad_bn_fuses(k, B, H, W, Nf, ksize, c.dtype);
    if (bz && k.d1 && !(c.exclude & Y2X_D1) && y2_d1_shape(Cp, c.ldp, Nf, c.ldo, ksize, c.dtype, M) && (c.align & Y2A_O16) && (c.align & Y2A_Y16)) {
        // 1x1 data gradient of the wide early stages (conv3 / conv6): persistent kernel with prefetched y vectors and launch-long sums (conv_d1.hip)
        const Y2PersistentPlan pl = y2_d1_plan(M, Nf, cus);
        if (pl.grid) {
            r.stats = Y2S_EPILOGUE; r.kernel_stats = true; r.pending = 1;
            return take(Y2F_D1, pl.grid, Nf / 128, pl.rows, {128, 128, 8, Cp / 8, 1, 0x100, pl.rows, Nf / 128});
        }
    }
    const int MT = cdiv(M, 128), BK = 4 * VEC, WIDE_K = 8 * VEC;      // channels of a 64- / 128-byte K row
    const bool ctail = (Cp % BK) != 0;
    // 16-byte epilogue stores need 16-byte aligned pixel rows, and a partial last chunk may only spill into this tensor's own
    // padding lanes (written as zeros), never into a neighbouring concat slice
    r.wide_store = (c.align & Y2A_O16) && c.ldo % VEC == 0 && (Nf % VEC == 0 || c.ldo < Nf + VEC);
    // XCD mapping: filter operand small -> contiguous M runs per XCD; else filter tiles pinned per XCD
    r.remap = (size_t)Nf * ksize * ksize * Cp * (is_bf16 ? 2 : 4) <= (3u << 19) ? 1 : 0;
    const int MT2 = cdiv(M, 256), NT2 = cdiv(Nf, 128);
    const long nk_wide = (Cp % WIDE_K == 0) ? (long)ksize * ksize * (Cp / WIDE_K) : 0;
    // stream-K of any kind: a workspace for the parked partial tiles, a flag per workgroup
    const bool stream_ok = k.stream && c.has_ws && cus <= Y2_STREAM_FLAG_WORDS && !(c.exclude & Y2X_FLAGS);
    // Ping-pong tap-fused kernel (conv_pp.hip): 3x3 layers on images up to 55 wide whose input is a multiple of 64 channels.  Its
    // fixed cost per launch (~24 us: prologue, stream-K hand-off, epilogue) against ~0.65 us per K step decides where it wins
    // (profiles/r04_pp2_*.txt, r04_pp3_*.txt, batch 16 and 8):
    //   * a tile grid that gives 60-100 % of the CUs one whole tile each: one workgroup per tile, no hand-off (26x26 256->512 forward
    //     30.8 vs 35.1 us; 52x52 data gradients 31 vs 36.5 us);
    //   * else stream-K over one workgroup per CU when a workgroup's share is >= 24 K steps and a tile is cut into at most four shares
    //     (the owner adds its partners' parked partials one after the other: the 13x13 512 -> 1024 forward, 88 tiles, 38.9 vs 41.0 us;
    //     its data gradient, 44 tiles of the same 24.75 steps per workgroup, 42.4 vs 41.1 us: per-tap; >= 1024-channel 13x13 layers
    //     55 vs 60-75 us, 126 vs 144-181 us);
    //   * a data gradient that also reduces the producer's BN-backward sums takes it from 10 steps per workgroup when it has >= 8192
    //     pixels: the per-tap kernels' form of that epilogue costs 12-30 us there, this one 4-7.
    if (is_bf16 && k.tap != 0 && !(c.exclude & Y2X_PP) && ksize == 3 && Cp % 64 == 0 && y2_pp_fits(W) && Nf > 64 && r.wide_store && stream_ok &&
        (long)9 * (Cp / 64) >= k.pp_min_steps) {
        const long tiles_t = (long)MT2 * NT2, units_p = tiles_t * 9 * (Cp / 64);
        const int gm = k.pp_grid;
        const bool can_stream = stream_ws_bytes(cus, 256) <= c.ws_bytes;
        long grid = 0;
        if (gm == 1) grid = can_stream ? cus : 0;
        else if (gm == 2) grid = tiles_t <= Y2_STREAM_FLAG_WORDS ? tiles_t : 0;
        else if (gm >= 8) grid = (can_stream && gm <= cus) ? gm : 0;                  // explicit workgroup count (sweeps)
        else if (gm <= -2) grid = (can_stream && tiles_t * -gm <= cus) ? tiles_t * -gm : 0;      // -P: every tile cut into exactly P shares
        else if (tiles_t * 10 >= (long)cus * 6 && tiles_t <= cus) grid = tiles_t;
        else if (can_stream && ((units_p >= k.pp_min_share * cus && tiles_t * 4 >= cus) || (bz && M >= 8192 && units_p >= 10L * cus) ||
                                // long shares (>= 26 steps per workgroup) outweigh a tile cut into 5-8 of them -- batch 8, 48 tiles: conv20
                                // forward 79 vs 119 us, conv18 41.2 vs 44.6 (profiles/r04_pp6_b8.txt); the COCO-80 batch-8 step 2.84 -> 2.82 ms
                                // (profiles/r05_long_share_b8.txt)
                                (k.pp_long_share > 0 && units_p >= (long)k.pp_long_share * cus && tiles_t * 8 >= cus))) grid = cus;
        // every workgroup of a stream-K launch must hold at least one K step: an owner waits for the flag of EVERY workgroup whose range
        // lies inside its tile, and one without work never raises it (only a forced grid on a tiny problem gets here: the rule above
        // asks for >= 10 steps per workgroup)
        if (grid > units_p && !k.sk_unclamped) grid = units_p;
        if (grid > 0) {
            r.family = (k.tap == 3 && !(c.exclude & Y2X_S4)) ? Y2F_S4 : Y2F_PP;
            r.grid_x = (int)grid; r.NT = NT2; r.use_ws = r.flags = true;
            // partial rows per pixel tile: what the kernel that runs indexes (conv_shared.h)
            const int tile_rows = r.family == Y2F_S4 ? (bz ? Y2S_STAT_ROWS_BNBWD : Y2S_STAT_ROWS_FWD) : (bz ? Y2P_STAT_ROWS_BNBWD : Y2P_STAT_ROWS_FWD);
            set_stat_rows(r, (long)MT2 * tile_rows, Nf, VEC);
            // owner cost of the cost-balanced partition: below half a workgroup's share, so that every workgroup keeps real K steps (an owner
            // waits for the flag of every workgroup inside its tile); whole-tile grids have no shares to balance
            r.cv = (int)std::min<long>(grid == tiles_t ? 0 : k.pp_cv, units_p / grid / 2);
            if (bz) { r.stats = Y2S_EPILOGUE; r.kernel_stats = true; r.pending = 1; }
            // "stages" 18: nine taps per halo image, two phases per tap; waves: the COMPUTING waves (s4: + four loaders); grid_y bits 8..: the owner cost
            set_plan({256, 128, r.family == Y2F_S4 ? 4 : 8, 8, 18, bz ? 0x102 : 2, r.grid_x, 1 + (r.cv << 8)});
            return r;
        }
    }
    r.family = Y2F_IGEMM;
    Y2IgemmKey &ig = r.ig;
    auto key = [&](int BM, int BN, int WGN, int stages, int split, bool ct, int chunks, int waves) { ig = Y2IgemmKey{c.dtype, BM, BN, WGN, stages, ksize, split, ct, chunks, waves, 0}; };
    // Long reductions on under-filled grids (13x13 stages: 1024+ input channels): 256 x 128 tile, 8 waves of 64 x 64
    // (half the LDS fragment traffic and 25 % less DMA per flop than 32 x 64 per wave), always stream-K.  Measured
    // (profiles/r01_igemm_bm256.txt): +23 % on the 3072-channel layer; shorter reductions, fuller grids and grids under
    // 64 tiles (each tile cut into > 4 parts: the owner's serial fix-up) lose.
    if (Nf > 64 && stream_ok && nk_wide >= 128 && MT2 * NT2 >= 64 && MT2 * NT2 <= 3 * cus && stream_ws_bytes(cus, 256) <= c.ws_bytes) {
        key(256, 128, 2, 3, 2, false, 8, 8);
        r.NT = NT2; r.grid_x = cus; r.use_ws = r.flags = true;
    } else if (Nf > 64) {
        // 128 x 128 tile, 8 waves (4 x 2, each 32 x 64): two waves per SIMD even when a CU holds a single workgroup.
        // Grids of <= 256 tiles (the 13x13 / 26x26 stages at batch 16) cannot fill the chip with workgroups, so they
        // take 128-byte K rows (16 MFMAs per wave between barriers, 96 KiB ring, one workgroup per CU); larger grids
        // keep 64-byte rows (48 KiB ring, 3 workgroups per CU).  Measured in profiles/r01_igemm_variants.txt.
        const int NT = r.NT = cdiv(Nf, 128);
        // K slicing (grids <= 128 tiles with a long reduction) multiplies the workgroup count, so it pairs with the
        // narrow variant (3 workgroups per CU); unsliced small grids take the wide one.
        // (deterministic mode: no K slicing -- its slices meet in f32 atomics; stream-K or the unsplit grid instead)
        int ks = (c.has_ws && !c.deterministic) ? choose_ksplit((long)MT * NT, ksize * ksize * cdiv(Cp, BK)) : 1;
        if (ks > 1 && (size_t)M * Nf * sizeof(float) > c.ws_bytes) ks = 1;
        const bool wide = ks == 1 && MT * NT <= 256 && Cp % WIDE_K == 0;
        // stream-K: a grid that cannot give every CU a tile (13x13 stages at batch 16: 176 tiles, 88 for the narrower
        // data gradients) is run by exactly one 8-wave wide-row workgroup per CU, each taking an equal contiguous share
        // of the flat (tile, K step) space (>= 24 K steps each, else the two partial-tile epilogues dominate).  Grids of
        // 1-3 tiles per CU gain only when the reduction is long (>= 96 K steps per tile; measured, profiles/)
        const long units = (long)MT * NT * ksize * ksize * (Cp / WIDE_K);
        if (stream_ok && Cp % WIDE_K == 0 && units >= 24L * cus && (MT * NT < cus || (MT * NT <= 3 * cus && units / (MT * NT) >= 96)) &&
            stream_ws_bytes(cus, 128) <= c.ws_bytes) {
            key(128, 128, 2, 3, 2, false, 8, 8);
            r.grid_x = cus; r.use_ws = r.flags = true;
        } else if (ks > 1) {        // partial tiles meet only in the finishing kernel: statistics from a pass over the finished output
            key(128, 128, 2, 3, 1, ctail, 4, 4);     // 4-wave workgroups: 3 per CU, measured best with slicing
            r.grid_x = MT * NT; r.grid_y = ks; r.use_ws = r.memset_ws = r.finish = true;
        } else {
            r.grid_x = MT * NT;
            if (wide) key(128, 128, 2, 3, 0, false, 8, 8);
            // full grids with >= 64 channels: 128-byte rows on a 2-stage ring (64 KiB: two workgroups per CU, 8 MFMAs per
            // wave between barriers instead of 4) -- +8..19 % on the 52x52 / 26x26 stages (profiles/r01_igemm_wide_ns2.txt)
            else if (Cp % WIDE_K == 0) key(128, 128, 2, 2, 0, false, 8, 8);
            else key(128, 128, 2, 3, 0, ctail, 4, 8);
        }
    } else {
        r.NT = 1; r.grid_x = MT;
        const int BN = Nf > 32 ? 64 : 32;
        // 3x3 with <= 64 filters and >= 64 channels (the 208x208 / 104x104 data gradients): 128-byte rows, 2-stage ring;
        // +35 % / +20 % on those two launches; the 1x1 layers measured no gain (profiles/r01_igemm_wide_ns2.txt)
        if (ksize == 3 && Cp % WIDE_K == 0) key(128, BN, 1, 2, 0, false, 8, 4);
        else key(128, BN, 1, 3, 0, ctail, 4, 4);
    }
    const Y2IgemmLine *g = r.line = y2_igemm_line(ig);
    if (!g) return r;
    // does this instantiation have the fused BN-backward epilogue?  (else it has no on-chip tile image to reduce from: the two-step form)
    const bool fusedbw = bz && ig.split != 1 && !ctail && r.wide_store && g->wide_fits;
    set_stat_rows(r, (long)cdiv(M, ig.BM) * (fusedbw ? g->rows_bnbwd : g->rows_fwd), Nf, VEC);
    if (fusedbw) { ig.bnbwd = 1; r.line = y2_igemm_line(ig); r.stats = Y2S_EPILOGUE; r.kernel_stats = true; r.pending = 1; }
    else if (bz) r.stat_mask_inv = 0;      // (a plain launch: nothing reads the mask)
    if (bn && ig.split == 1) { r.stats = Y2S_COLSUM; r.stat_rows = y2_colsum_rows(M, Nf, c.dtype); }
    set_plan({ig.BM, ig.BN, ig.waves, ig.chunks, ig.stages, ig.split | (fusedbw ? 0x100 : 0), r.grid_x, r.grid_y});
    return r;
}

// the plan of the calling thread's most recent launch (yolo2_debug_last_conv_plan): tests assert that the variant they
// mean to check is the one that ran, since the choice is shape-driven.  y2_conv_launch copies both from the route.
static thread_local int g_last_plan[8] = {0, 0, 0, 0, 0, 0, 0, 0};
static thread_local int g_last_stat_rows = Y2_BN_PART_ROWS;
extern "C" int yolo2_last_bn_part_rows(void) { return g_last_stat_rows; }
extern "C" int yolo2_debug_last_conv_plan(int *out8) {
    if (out8) std::copy(g_last_plan, g_last_plan + 8, out8);
    return out8 ? YOLO2_OK : YOLO2_E_ARG;
}

struct Y2ConvPtrs {      // the pointers and scalars of a call that the rule does not read
    const void *P, *F; const float *bias; void *O; float *ws; const float *bn_shift; float *bn_part; float act_alpha;
    const Y2BnBwd *bwd; float *dgamma, *dbeta; double *red_ws; int *pending;
};

// Launches what `r` names.  -> YOLO2_OK / an error code; *refused: the Y2X_* bit of a feature that only now turned out to be unavailable (nothing was
// launched: the caller excludes it and routes again)
static int y2_conv_launch(const Y2ConvRoute &r, const Y2ConvCall &c, const Y2ConvPtrs &p, hipStream_t st, const char *fn, unsigned *refused) {
    const long M = (long)c.B * c.H * c.W;
    const size_t esz = c.dtype == YOLO2_BF16 ? 2 : 4;
    const unsigned p_bytes = (unsigned)((size_t)M * c.ldp * esz), f_bytes = (unsigned)((size_t)c.Nf * c.ksize * c.ksize * c.Cp * esz);
    unsigned *sk_flags = nullptr;
    if (r.flags && !(sk_flags = y2_stream_flags())) { *refused = Y2X_FLAGS; return YOLO2_OK; }
    float *part = r.kernel_stats ? p.bn_part : nullptr;
    Y2BnBwd bz = (r.stats == Y2S_EPILOGUE && p.bwd) ? *p.bwd : Y2BnBwd{nullptr, nullptr, nullptr, nullptr, nullptr, 0.f, 0.f, 0};
    bz.stat_mask_inv = r.stat_mask_inv;
    int refusal = 0;      // non-zero: the family's launcher declined (nothing was launched)
    switch (r.family) {
    case Y2F_FIRST: y2_first_layer_fwd(p.P, p.F, p.O, c.B, c.H, c.W, c.dtype, st, p.bn_shift, p.bn_part); break;
    case Y2F_C32: refusal = y2_c32_fwd(p.P, p.F, p.O, c.B, c.H, c.W, p.bias, p.act_alpha, p.bn_shift, p.bn_part, c.cus, st) ? Y2X_C32 : 0; break;
    case Y2F_C64: refusal = y2_c64_fwd(p.P, p.F, p.O, c.B, c.H, c.W, c.Nf, p.bias, p.act_alpha, p.bn_shift, p.bn_part, c.cus, st) ? Y2X_C64 : 0; break;
    case Y2F_D1: refusal = y2_d1_dgrad_bn(p.P, p.F, p.O, M, c.Cp, c.Nf, p.bn_part, bz, c.cus, st) ? Y2X_D1 : 0; break;
    case Y2F_S4:
        refusal = y2_conv3x3_s4_launch(p.P, p_bytes, p.F, f_bytes, p.bias, p.O, p.ws, c.H, c.W, c.Cp, c.ldp, c.Nf, c.ldo, (int)M, r.NT, p.bn_shift, part, sk_flags,
                                       p.act_alpha, bz, 1, r.grid_x, c.knobs.s4_abl, st) ? Y2X_S4 : 0;
        break;
    case Y2F_PP:
        refusal = y2_conv3x3_pp_launch(p.P, p_bytes, p.F, f_bytes, p.bias, p.O, p.ws, c.H, c.W, c.Cp, c.ldp, c.Nf, c.ldo, (int)M, r.NT, p.bn_shift, part, sk_flags,
                                       p.act_alpha, bz, /* K rotation of the stream-K tiles (profiles/r03_l2_stationary_ab.md) */ 1, r.grid_x, c.knobs.pp_sched,
                                       r.cv, st) ? Y2X_PP : 0;
        break;
    default: {
        const Y2IgemmKey &k = r.ig;
        if (!r.line) {      // (checked before anything is enqueued)
            yolo2_set_error("%s: no conv_igemm_kernel instantiation (dtype %d, BM %d, BN %d, WGN %d, stages %d, KS %d, split %d, ctail %d, chunks %d, waves %d, bnbwd %d)",
                            fn, k.dtype, k.BM, k.BN, k.WGN, k.stages, k.KS, k.split, k.ctail, k.chunks, k.waves, k.bnbwd);
            return YOLO2_E_LAUNCH;
        }
        if (r.memset_ws && hipMemsetAsync(p.ws, 0, (size_t)M * c.Nf * sizeof(float), st) != hipSuccess) { yolo2_set_error("%s: workspace memset failed", fn); return YOLO2_E_LAUNCH; }
        r.line->launch(r.grid_x, r.grid_y, Y2IgemmArgs{p.P, p_bytes, p.F, f_bytes, p.bias, p.O, r.use_ws ? p.ws : nullptr, c.H, c.W, c.Cp, c.ldp, c.Nf, c.ldo, (int)M, r.NT,
                                                       r.remap, p.bn_shift, part, sk_flags, p.act_alpha, r.wide_store, bz}, st);
        if (r.finish) y2_splitk_finish(p.ws, p.bias, p.O, M, c.Nf, c.ldo, p.act_alpha, c.dtype, st);
    }
    }
    if (refusal) { *refused = refusal; return YOLO2_OK; }
    std::copy(r.plan, r.plan + 8, g_last_plan);
    if (r.stat_rows) g_last_stat_rows = r.stat_rows;
    Y2_CHECK_LAUNCH();
    if (c.mode == Y2M_DGRAD_BN) {
        if (p.pending) *p.pending = r.pending;
        if (r.stats == Y2S_EPILOGUE) return p.pending ? YOLO2_OK : y2_bn_part_to_grads(p.bn_part, c.Nf, p.dgamma, p.dbeta, st);
        return yolo2_bn_leaky_bwd_reduce(p.O, c.ldo, p.bwd->Y, p.bwd->mean, p.bwd->var, p.bwd->gamma, p.bwd->beta, p.dgamma, p.dbeta, p.red_ws, M, c.Nf,
                                         p.bwd->eps, p.bwd->alpha, c.dtype, st);
    }
    if (r.stats == Y2S_COLSUM) return y2_colsum_into(p.O, c.ldo, M, c.Nf, p.bn_shift, p.bn_part, c.dtype, st);
    return YOLO2_OK;
}

static int conv2d_impl(const void *P, const void *F, const float *bias, void *O, float *ws, size_t ws_bytes, int B, int H, int W, int Cp, int ldp, int Nf, int ldo,
                       int ksize, int dtype, void *stream, const char *fn, const float *bn_shift = nullptr, float *bn_part = nullptr, float act_alpha = 1.0f, const Y2BnBwd *bwd = nullptr,
                       float *dgamma = nullptr, float *dbeta = nullptr, double *red_ws = nullptr, int *pending = nullptr) {
    if (!(P && F && O) || !(B > 0 && H > 0 && W > 0 && Cp > 0 && Nf > 0) || !(ksize == 1 || ksize == 3) || !(ldp >= Cp && ldo >= Nf))
        { yolo2_set_error("%s: argument check failed: pointers / extents / ksize / strides", fn); return YOLO2_E_ARG; }
    if (dtype != YOLO2_F32 && dtype != YOLO2_BF16) { yolo2_set_error("%s: bad dtype %d", fn, dtype); return YOLO2_E_ARG; }
    const int vec = dtype == YOLO2_BF16 ? 8 : 4, esz = 16 / vec;
    // the DMA path addresses both operands with 32-bit byte offsets below 2^31
    // (only the two DMA-read operands; the output is addressed with 64-bit pointers)
    if ((size_t)B * H * W * (size_t)ldp * esz >= (1ull << 31) || (size_t)Nf * ksize * ksize * Cp * esz >= (1ull << 31) || (size_t)B * H * W >= (1ull << 31) ||
        Cp % vec || ldp % vec || ((uintptr_t)P & 15) || ((uintptr_t)F & 15))
        { yolo2_set_error("%s: argument check failed: operand >= 2 GiB or misaligned (channels must be a multiple of %d)", fn, vec); return YOLO2_E_ARG; }
    const int mode = bwd ? Y2M_DGRAD_BN : bn_part ? Y2M_BN_FWD : (bias || act_alpha != 1.0f) ? Y2M_BIAS_ACT : Y2M_PLAIN;
    const int align = (((uintptr_t)O & 15) == 0 ? Y2A_O16 : 0) | (((uintptr_t)F & 15) == 0 ? Y2A_F16 : 0) | ((bwd && ((uintptr_t)bwd->Y & 15) == 0) ? Y2A_Y16 : 0);
    Y2ConvCall call{B, H, W, Cp, ldp, Nf, ldo, ksize, dtype, mode, align, ws != nullptr, ws_bytes, yolo2_get_stream_workgroups(), y2_deterministic() != 0, 0u, knobs_now()};
    const Y2ConvPtrs ptrs{P, F, bias, O, ws, bn_shift, bn_part, act_alpha, bwd, dgamma, dbeta, red_ws, pending};
    for (;;) {      // (at most once more per feature the runtime refuses)
        unsigned refused = 0;
        const int rc = y2_conv_launch(y2_conv_route(call), call, ptrs, (hipStream_t)stream, fn, &refused);
        if (!refused) return rc;
        call.exclude |= refused;
    }
}

extern "C" int yolo2_conv2d_dgrad_bn_fuses(int B, int H, int W, int Nf, int ksize, int dtype) {
    return (B > 0 && H > 0 && W > 0 && Nf > 0 && (dtype == YOLO2_F32 || dtype == YOLO2_BF16) && y2_dgrad_bn_fuses(knobs_now(), B, H, W, Nf, ksize, dtype)) ? 1 : 0;
}

extern "C" size_t yolo2_conv2d_workspace_bytes(int B, int H, int W, int Cp, int Nf, int ksize, int dtype) {
    // the largest scratch any variant of yolo2_conv2d_ws / _bn / _bias_leaky can use for this shape: one f32 256x128 tile slot
    // per CU (stream-K) or the f32 [M][Nf] partial-sum image (K-sliced grids); smaller buffers only disable variants
    if (!(B > 0 && H > 0 && W > 0 && Cp > 0 && Nf > 0) || !(dtype == YOLO2_F32 || dtype == YOLO2_BF16)) return 0;
    const size_t M = (size_t)B * H * W, slots = stream_ws_bytes(default_stream_wgs(), 256), image = M * Nf * sizeof(float);
    const int ks = choose_ksplit((long)cdiv((long)M, 128) * cdiv(Nf, 128), ksize * ksize * cdiv(Cp, dtype == YOLO2_BF16 ? 32 : 16));
    return ks > 1 && image > slots ? image : slots;
}

// The route of a call, without a device: out12 = the eight plan words, partial rows (0: none written), statistics source (Y2S_*), pending, family.
// cus <= 0: the process's current workgroup count (the one input that may ask the runtime); the knobs and the calling thread's deterministic flag are
// read as a launch would read them.
extern "C" int yolo2_debug_conv_route(int B, int H, int W, int Cp, int ldp, int Nf, int ldo, int ksize, int dtype, int mode, int align_bits, size_t ws_bytes,
                                      int cus, unsigned exclude, int *out12) {
    if (!out12 || !(B > 0 && H > 0 && W > 0 && Cp > 0 && Nf > 0) || !(ksize == 1 || ksize == 3) || !(dtype == YOLO2_F32 || dtype == YOLO2_BF16) ||
        mode < Y2M_PLAIN || mode > Y2M_DGRAD_BN)
        { yolo2_set_error("yolo2_debug_conv_route: argument check failed"); return YOLO2_E_ARG; }
    const Y2ConvCall call{B, H, W, Cp, ldp, Nf, ldo, ksize, dtype, mode, align_bits, ws_bytes > 0, ws_bytes, cus > 0 ? cus : yolo2_get_stream_workgroups(),
                          y2_deterministic() != 0, exclude, knobs_now()};
    const Y2ConvRoute r = y2_conv_route(call);
    std::copy(r.plan, r.plan + 8, out12);
    out12[8] = r.stat_rows; out12[9] = r.stats; out12[10] = r.pending; out12[11] = r.family;
    return YOLO2_OK;
}

extern "C" int yolo2_conv2d(const void *P, const void *F, const float *bias, void *O, int B, int H, int W, int Cp, int ldp, int Nf, int ldo, int ksize, int dtype, void *stream) {
    return conv2d_impl(P, F, bias, O, nullptr, 0, B, H, W, Cp, ldp, Nf, ldo, ksize, dtype, stream, "yolo2_conv2d");
}

extern "C" int yolo2_conv2d_bn(const void *P, const void *F, void *O, float *ws, size_t ws_bytes, int B, int H, int W, int Cp, int ldp,
                               int Nf, int ldo, int ksize, const float *shift, float *bn_part, int dtype, void *stream) {
    if (!shift || !bn_part || ldo != Nf) { yolo2_set_error("yolo2_conv2d_bn: argument check failed: shift / bn_part NULL or ldo != Nf"); return YOLO2_E_ARG; }
    return conv2d_impl(P, F, nullptr, O, ws, ws_bytes, B, H, W, Cp, ldp, Nf, ldo, ksize, dtype, stream, "yolo2_conv2d_bn", shift, bn_part);
}

extern "C" int yolo2_conv2d_dgrad_bn(const void *dY, const void *F, void *dX, float *ws, size_t ws_bytes, int B, int H, int W, int Cp, int ldp,
                                     int Nf, int ldo, int ksize, const void *Yprev, const float *mean, const float *var, const float *gamma,
                                     const float *beta, float *dgamma, float *dbeta, float *bn_part, double *red_ws, float eps, float alpha,
                                     int *pending, int dtype, void *stream) {
    if (!Yprev || !mean || !var || !gamma || !beta || !dgamma || !dbeta || !bn_part || !red_ws) { yolo2_set_error("yolo2_conv2d_dgrad_bn: argument check failed: a producer-layer pointer is NULL"); return YOLO2_E_ARG; }
    const Y2BnBwd bz{Yprev, mean, var, gamma, beta, eps, alpha, 0};
    return conv2d_impl(dY, F, nullptr, dX, ws, ws_bytes, B, H, W, Cp, ldp, Nf, ldo, ksize, dtype, stream, "yolo2_conv2d_dgrad_bn", nullptr, bn_part, 1.0f,
                       &bz, dgamma, dbeta, red_ws, pending);
}
extern "C" int yolo2_bn_part_to_grads(float *bn_part, int C, float *dgamma, float *dbeta, void *stream) {
    if (!bn_part || !dgamma || !dbeta || C <= 0) { yolo2_set_error("yolo2_bn_part_to_grads: argument check failed"); return YOLO2_E_ARG; }
    return y2_bn_part_to_grads(bn_part, C, dgamma, dbeta, (hipStream_t)stream);
}

extern "C" int yolo2_conv2d_bias_leaky(const void *P, const void *F, const float *bias, void *O, float *ws, size_t ws_bytes, int B, int H, int W,
                                       int Cp, int ldp, int Nf, int ldo, int ksize, float alpha, int dtype, void *stream) {
    if (!bias) { yolo2_set_error("yolo2_conv2d_bias_leaky: bias is NULL"); return YOLO2_E_ARG; }
    return conv2d_impl(P, F, bias, O, ws, ws_bytes, B, H, W, Cp, ldp, Nf, ldo, ksize, dtype, stream, "yolo2_conv2d_bias_leaky", nullptr, nullptr, alpha);
}

extern "C" int yolo2_conv2d_ws(const void *P, const void *F, const float *bias, void *O, float *ws, size_t ws_bytes, int B, int H, int W, int Cp, int ldp, int Nf, int ldo, int ksize, int dtype, void *stream) {
    return conv2d_impl(P, F, bias, O, ws, ws_bytes, B, H, W, Cp, ldp, Nf, ldo, ksize, dtype, stream, "yolo2_conv2d_ws");
}
