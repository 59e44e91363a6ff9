// NHWC implicit-GEMM convolution on MFMA (gfx950), forward and data-gradient.
//
// Replaces slim.layers.conv2d (reference model/yolo2/inference.py:37-48,73-118) and its
// tf.gradients input-gradient (train.py:127-129).
//
//   O[m, n] = bias[n] + sum_{tap, c} P[pix(m) + shift(tap), c] * F[n][tap*Cp + c]
//   GEMM view: M = B*H*W output pixels, N = Nf filters, K = ksize^2 * Cp.
//
//   K order of a filter row: 64-channel chunk, tap, channel (common.h y2_filter_koff): the 9 shifted re-reads of a
//   pixel-tile x 64-channel slab are consecutive K steps and hit in the XCD's L2.
//
// Structure (one workgroup = NW waves = a BM(M) x BN(N) output tile; a K step = CH 16-byte chunks of one tap's channels):
//   * Operands go HBM/L2 -> LDS by DMA: buffer_load_dwordx4 ... lds (1 KiB per wave-instruction, no
//     VGPR round trip, no ds_write pass).  The DMA writes LDS lane-linearly (wave-uniform base +
//     lane*16 B), so rows cannot be padded; the b128 fragment reads are kept bank-conflict-free by an
//     XOR swizzle applied on the SOURCE side: the lane that owns LDS position (row, slot) fetches global
//     chunk  slot ^ ((row / rows_per_256B) % CH); the fragment reads apply the same involution
//     (SQ_LDS_BANK_CONFLICT = 0 measured).
//   * SAME padding, image borders, the M tail, filter-row tail and channel tail are all realised by the
//     buffer descriptor's hardware range check: a lane that must contribute zeros uses an out-of-range
//     offset and the DMA writes 0 -- no branches, no pointer selects, 32-bit offsets only.  Which of the
//     9 taps are inside the image for a pixel row is a 9-bit mask (outer product of a row and a column 3-bit set)
//     computed once per lane per tile, with reciprocal-multiply pixel decoding (no hardware integer divider).
//     Instruction overhead per MFMA decided the short-reduction layers twice: the first version spent 11 VALU + 12 SALU
//     per MFMA on per-piece address arithmetic (17 % MFMA utilisation); later the tile prologue's divisions and the
//     per-element row test of the epilogue cost conv1..conv8 15-35 %.
//   * NSTAGE-deep LDS ring: the DMA of tile t+NSTAGE-1 is issued right after the barrier of tile t and
//     only tile t's own pieces are waited for (counted s_waitcnt vmcnt(N) + raw s_barrier; a
//     __syncthreads() would drain every DMA in flight).
//   * A = pixels (rows), B = filters (cols): the 32x32 accumulator layout puts 32 consecutive output
//     channels of one pixel in 32 consecutive lanes -> 64 B (bf16) / 128 B (f32) store segments.
//   * Shapes (chosen per layer from measurements: conv_route.hip y2_conv_route): 128x128 tile, 8 waves, 128-byte K rows on a 2-stage
//     ring (64 KiB: two workgroups per CU, 8 MFMAs per wave between barriers) for full grids; 64-byte rows / 3 stages
//     when the channel count is not a multiple of 64; 64- and 32-filter tiles for the narrow layers.
//   * Under-filled grids (13x13 / 26x26 stages at batch 16: 88-176 tiles for 256 CUs) run stream-K: one workgroup per CU,
//     equal contiguous shares of the flat (tile, K step) space, partial tiles parked in the workspace and fixed up by
//     the tile's owner through sc1 (agent-coherent, fence-free) accesses -- see the SPLITK == 2 epilogue; long
//     reductions take a 256x128 tile (8 waves of 64x64, 16 MFMAs per barrier).  Grids <= 128 tiles with a medium
//     reduction slice the K loop over gridDim.y with f32 atomics + a finishing kernel (SPLITK == 1).
//   * The epilogue can also emit the batch-norm partial sums of the stored outputs (yolo2_conv2d_bn), apply
//     bias + leaky ReLU (yolo2_conv2d_bias_leaky, BN-folded inference), and -- for a data gradient whose output is the gradient of a
//     batch-normalised producer layer -- reduce that layer's dgamma / dbeta sums from the tile image (yolo2_conv2d_dgrad_bn).
//   * 3x3 layers with >= 1024 input channels on images up to 55 wide take conv3x3_tap_kernel (further down): one halo image per
//     64-channel chunk serves all nine taps, software-pipelined K loop.  Its stream-K tiles walk their 64-channel chunks in a
//     ROTATED order so that the ~32 workgroups of an XCD read the same bytes of a filter slab (7 MB > the 4 MB L2) at the same
//     time: 3.6x less fabric traffic on the 3072-channel layer (profiles/r03_l2_stationary_ab.md; the time moved 1.8 %: issue-bound).
//   * Statistics rows: a producer leaves one partial row per (pixel tile, wave row) while that is no more than the consumer's
//     prologue reads (conv_route.hip set_stat_rows: 128 rows for >= 128 bf16 channels), else it wraps around 16-128 rows with f32 atomics; the
//     kernel that consumes the moments finishes them (bn.hip *_fin kernels) -- no finalisation launch.
//   * blockIdx -> tile: filter tile fastest (the blocks of XCD b%8 keep one filter slab in their L2), or,
//     when the filter operand is small, one contiguous run of M tiles per XCD (halo rows shared in L2).
#include "common.h"
#include "conv_shared.h"
#include "conv_epilogue.h"
#include "conv_igemm_table.h"
#include <stdlib.h>
#include <string.h>
#include <atomic>
#include <mutex>
#include <type_traits>

template <typename T> struct Mma;
template <> struct Mma<bf16> {
    static constexpr int KSTEP = 16;
    typedef bf16x8 Frag;
    static __device__ __forceinline__ f32x16 mma(Frag a, Frag b, f32x16 c) {
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
    }
};
template <> struct Mma<float> {
    static constexpr int KSTEP = 2;
    typedef float Frag;
    static __device__ __forceinline__ f32x16 mma(Frag a, Frag b, f32x16 c) {
        return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
    }
};

// (Timing-ablation hooks -- no epilogue / no MFMA / no fragment reads / no DMA builds -- live in scripts/experiments/conv_igemm_ablation_hooks.patch,
// applied to a COPY of this file by scripts/abl_build.sh; the product source carries none.)
// (Y2_STREAM_FLAG_WORDS, conv_shared.h: one stream-K flag word per workgroup in a library-owned pool; the workspace holds one f32 tile slot each)
// SPLITK: 0 = one workgroup per output tile; 1 = K loop sliced over gridDim.y; 2 = stream-K: gridDim.x workgroups (one per
// CU) share the flat (tile, K step) space in equal contiguous ranges.  1 and 2 accumulate f32 partial tiles with atomics.
template <typename T, int BN, int WGN, int NSTAGE, int KS, int SPLITK, bool CTAIL, int CH = 4, int NW = 4, int BMv = 128, bool BNBWD = false>
__global__ __launch_bounds__(NW * 64) void conv_igemm_kernel(
    const T *__restrict__ P, unsigned p_bytes, const T *__restrict__ F, unsigned f_bytes, const float *__restrict__ bias,
    T *__restrict__ O, float *__restrict__ Oacc, int H, int W, int Cp, int ldp, int Nf, int ldo, int M, int NT, int remap,
    const float *__restrict__ bn_shift, float *__restrict__ bn_part, unsigned *__restrict__ sk_flags, float act_alpha, int wide_store,
    const Y2BnBwd bz) {
    constexpr int BM = BMv;                // pixels per tile: 128, or 256 (8 waves of 64 x 64)
    typedef Y2IgemmPlan<T, BM, BN, WGN, NSTAGE, CH, NW> Plan;      // (conv_shared.h: the sizes the host counts partial rows from)
    constexpr int TAPS = KS * KS;
    constexpr int VEC = Plan::VEC;
    constexpr int BK = CH * VEC;           // CH = 16-byte chunks per tile row: 4 -> 32 bf16 / 16 f32 per K step
    constexpr int ROWB = Plan::ROWB;       // bytes per tile row
    constexpr int RPL = 256 / ROWB;        // rows per 256-byte LDS bank line
    constexpr int RPI = Plan::RPI;         // rows per DMA instruction (1 KiB)
    constexpr int WGM = Plan::WGM, TM = Plan::TM, TN = Plan::TN;      // waves WGM x WGN over the output tile, TM x TN MFMA blocks each
    constexpr int A_IT = BM / RPI / NW;    // DMA instructions per wave per tile
    constexpr int B_PIECES = BN / RPI;
    constexpr int B_IT = Plan::B_IT;
    constexpr int LOADS = A_IT + B_IT;   // counted on vmcnt; identical in every wave (idle B slots still issue, all-OOB)
    constexpr int PAD = KS / 2;
    constexpr int STAGE = Plan::STAGE;
    static_assert(A_IT >= 1, "at least one A piece per wave");
    static_assert(NSTAGE >= 2 && NSTAGE <= 4 && TM >= 1 && TN >= 1, "tile");

    __shared__ __attribute__((aligned(1024))) unsigned char smem[NSTAGE * STAGE];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WGN, wn = wave % WGN;
    const int MT = (M + BM - 1) / BM;
    // K order (common.h y2_filter_koff): channel chunk, tap, BK-wide step inside the chunk
    const int KC = y2_kchunk(Cp, TAPS);
    const int kpc = (KC + BK - 1) / BK;   // K tiles per (chunk, tap)
    const int nk = (Cp / KC) * TAPS * kpc;
    // stream-K: this workgroup's range of the flat (tile, K step) space; workgroup b runs on XCD b % 8 and the
    // ranges of one XCD are contiguous, tiles ordered filter-tile-major (an XCD works on ~NT/8 filter slabs)
    long su = 0, su_end = 0, su_total = 0;
    int wx = 0;
    if (SPLITK == 2) {
        su_total = (long)MT * NT * nk;
        const int G = gridDim.x, b = blockIdx.x;
        wx = (G & 7) ? b : (b & 7) * (G >> 3) + (b >> 3);
        su = wx * su_total / G;
        su_end = (wx + 1) * su_total / G;
    }

    const __amdgpu_buffer_rsrc_t rsrcP = __builtin_amdgcn_make_buffer_rsrc(const_cast<T *>(P), 0, p_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsrcF = __builtin_amdgcn_make_buffer_rsrc(const_cast<T *>(F), 0, f_bytes, 0x00020000);
    const int lrow = lane / CH, lslot = lane % CH;
    const double rcp_hw = 1.0 / (double)(H * W);
    const float rcp_w = 1.0f / (float)W;

  for (bool first_seg = true;; first_seg = false) {
    int nt, mt, kt_beg = 0, kt_end = nk;
    if (SPLITK == 2) {
        if (su >= su_end) break;
        const int t = (int)(su / nk);
        kt_beg = (int)(su - (long)t * nk);
        kt_end = (int)min((long)nk, kt_beg + (su_end - su));
        su += kt_end - kt_beg;
        nt = t / MT;
        mt = t - nt * MT;
        if (!first_seg) __syncthreads();      // every wave is done reading the previous segment's LDS stages
    } else {
        int tile = blockIdx.x;
        if (remap) {   // one contiguous run of tiles per XCD (bijective for any grid size)
            const int ntile = gridDim.x, xcd = tile & 7, idx = tile >> 3, q = ntile >> 3, r = ntile & 7;
            tile = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
        }
        nt = tile % NT;
        mt = tile / NT;
        if (SPLITK == 1) {
            const int per = (nk + gridDim.y - 1) / gridDim.y;
            kt_beg = blockIdx.y * per;
            kt_end = min(nk, kt_beg + per);
            if (kt_beg >= kt_end) return;
        }
    }
    const int m0 = mt * BM, n0 = nt * BN;

    // per-lane source descriptors: byte offset of (row, swizzled chunk) and the set of taps inside the image
    unsigned a_voff[A_IT], a_mask[A_IT], a_cb[A_IT];
#pragma unroll
    for (int i = 0; i < A_IT; ++i) {
        const int r = (wave * A_IT + i) * RPI + lrow;
        a_cb[i] = (unsigned)((lslot ^ ((r / RPL) % CH)) * 16);   // byte offset of this lane's chunk inside the K step
        const int m = m0 + r;
        unsigned mask = 0;
        if (m < M) {
            // (b, h, w) of pixel m without integer division (no hardware divider: ~25 instructions each): reciprocal estimate
            // + one correction step.  m < 2^31 needs the f64 estimate (error << 1); rem < H*W < 2^24 is exact in f32.
            const int HW = H * W;
            int bq = (int)((double)m * rcp_hw);
            int rem = m - bq * HW;
            if (rem < 0) rem += HW; else if (rem >= HW) rem -= HW;
            int h = (int)((float)rem * rcp_w);
            int w = rem - h * W;
            if (w < 0) { w += W; --h; } else if (w >= W) { w -= W; ++h; }
            if (KS == 3) {      // tap (r, s) is inside the image iff row h+r-1 and column w+s-1 are: outer product of two 3-bit sets
                const unsigned cm = (w > 0 ? 1u : 0u) | 2u | (w < W - 1 ? 4u : 0u);
                mask = (h > 0 ? cm : 0u) | (cm << 3) | (h < H - 1 ? cm << 6 : 0u);
            } else {
                mask = 1u;
            }
        }
        a_mask[i] = mask;
        a_voff[i] = (unsigned)m * (unsigned)ldp * (unsigned)sizeof(T) + a_cb[i];
    }
    unsigned b_voff[B_IT], b_cb[B_IT];
#pragma unroll
    for (int i = 0; i < B_IT; ++i) {
        const int piece = wave * B_IT + i;
        const int r = piece * RPI + lrow;
        b_cb[i] = (unsigned)((lslot ^ ((r / RPL) % CH)) * 16);
        const int n = n0 + r;
        const bool ok = piece < B_PIECES && n < Nf;
        b_voff[i] = ok ? (unsigned)n * (unsigned)(KS * KS * Cp) * (unsigned)sizeof(T) + b_cb[i] : Y2_OOB;
    }

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    // issue cursor (wave-uniform scalars), NSTAGE-1 tiles ahead of the compute cursor
    int kt_issue = kt_beg;
    int i_chunk0 = (kt_beg / (TAPS * kpc)) * KC;            // first channel of the chunk
    int i_tap = (kt_beg / kpc) % TAPS;
    int i_c0 = i_chunk0 + (kt_beg % kpc) * BK;              // first channel of the step
    int i_dh = i_tap / KS - PAD, i_dw = i_tap % KS - PAD;
    int i_stage = 0;
    const unsigned cp_bytes = (unsigned)Cp * (unsigned)sizeof(T);
    auto issue_next = [&]() {
        const unsigned tapbit = 1u << i_tap;
        const unsigned offA = (unsigned)((i_dh * W + i_dw) * ldp + i_c0) * (unsigned)sizeof(T);   // may wrap: added mod 2^32
        const unsigned offB = (unsigned)(i_chunk0 * TAPS + i_tap * KC + (i_c0 - i_chunk0)) * (unsigned)sizeof(T);
        const unsigned c0b = (unsigned)i_c0 * (unsigned)sizeof(T);
        unsigned char *As = smem + i_stage * STAGE;
        unsigned char *Bs = As + BM * ROWB;
#pragma unroll
        for (int i = 0; i < A_IT; ++i) {
            bool ok = (a_mask[i] & tapbit) != 0;
            if (CTAIL) ok = ok && (c0b + a_cb[i] < cp_bytes);
            const unsigned voff = ok ? a_voff[i] + offA : Y2_OOB;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrcP, (__attribute__((address_space(3))) void *)(As + (wave * A_IT + i) * 1024), 16, voff, 0, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < B_IT; ++i) {
            unsigned voff = b_voff[i] + offB;           // an OOB row stays out of range: OOB + offB < 2^32 and >= 2^31
            if (CTAIL) voff = (c0b + b_cb[i] < cp_bytes) ? voff : Y2_OOB;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrcF, (__attribute__((address_space(3))) void *)(Bs + (wave * B_IT + i) * 1024), 16, voff, 0, 0, 0);
        }
        ++kt_issue;
        i_stage = (i_stage + 1 == NSTAGE) ? 0 : i_stage + 1;
        i_c0 += BK;
        if (i_c0 >= i_chunk0 + KC) {
            if (++i_tap == TAPS) { i_tap = 0; i_chunk0 += KC; i_dh = -PAD; i_dw = -PAD; }
            else if (++i_dw > PAD) { i_dw = -PAD; ++i_dh; }
            i_c0 = i_chunk0;
        }
    };
#pragma unroll
    for (int s = 0; s < NSTAGE - 1; ++s)
        if (kt_issue < kt_end) issue_next();

    // fragment read addressing: row i = lane&31 (+32 per MFMA tile); 32 rows = a whole number of swizzle periods
    const int frow = lane & 31;
    const int fsw = (frow / RPL) % CH;
    int c_stage = 0;
    for (int kt = kt_beg; kt < kt_end; ++kt) {
        // wait for tile kt only: up to NSTAGE-2 younger tiles stay in flight across the barrier
        const int ahead = min(NSTAGE - 2, kt_issue - 1 - kt);
        if (ahead >= 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * LOADS) : "memory");
        else if (ahead == 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(LOADS) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();      // tile kt complete in LDS for every wave; tile kt-1's buffer is free
        if (kt_issue < kt_end) issue_next();
        const unsigned char *As = smem + c_stage * STAGE + (wm * TM * 32 + frow) * ROWB;
        const unsigned char *Bs = smem + c_stage * STAGE + (BM + wn * TN * 32 + frow) * ROWB;
        c_stage = (c_stage + 1 == NSTAGE) ? 0 : c_stage + 1;
        // 128-byte rows, 8 waves of 32 x 64 (bf16): all twelve fragment reads of the K step are issued before its first MFMA (48 VGPRs)
        // and the MFMAs wait with a falling lgkmcnt; left to itself hipcc issues read, wait, MFMA, read, wait, MFMA ... and every
        // MFMA pair pays a full LDS latency (the tap-fused kernel below gained 15 % from the same change).
        constexpr bool HOIST = sizeof(T) == 2 && CH == 8 && NW == 8 && BM == 128;
        if constexpr (HOIST) {
            constexpr int KK = BK / Mma<T>::KSTEP;
            typename Mma<T>::Frag af[KK][TM], bf[KK][TN];
#pragma unroll
            for (int kk = 0; kk < KK; ++kk) {
                const int boff = ((kk * 2 + (lane >> 5)) ^ fsw) * 16;
#pragma unroll
                for (int i = 0; i < TM; ++i) af[kk][i] = *reinterpret_cast<const typename Mma<T>::Frag *>(As + i * 32 * ROWB + boff);
#pragma unroll
                for (int j = 0; j < TN; ++j) bf[kk][j] = *reinterpret_cast<const typename Mma<T>::Frag *>(Bs + j * 32 * ROWB + boff);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int kk = 0; kk < KK; ++kk)
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j) acc[i][j] = Mma<T>::mma(af[kk][i], bf[kk][j], acc[i][j]);
            __builtin_amdgcn_sched_barrier(0);
        } else
#pragma unroll
        for (int kk = 0; kk < BK / Mma<T>::KSTEP; ++kk) {
            typename Mma<T>::Frag af[TM], bf[TN];
            int boff;
            if constexpr (sizeof(T) == 2) {
                const int q = kk * 2 + (lane >> 5);            // 16-byte chunk holding this lane's 8 k values
                boff = (q ^ fsw) * 16;
            } else {
                const int e = kk * 2 + (lane >> 5);            // float index inside the row
                boff = (((e >> 2) ^ fsw) * 16) + (e & 3) * 4;
            }
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                af[i] = *reinterpret_cast<const typename Mma<T>::Frag *>(As + i * 32 * ROWB + boff);
            }
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                bf[j] = *reinterpret_cast<const typename Mma<T>::Frag *>(Bs + j * 32 * ROWB + boff);
            }
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    acc[i][j] = Mma<T>::mma(af[i], bf[j], acc[i][j]);
                }
        }
    }

    if (SPLITK == 2) {
        // Stream-K fix-up without atomics.  A workgroup's range is [tail of a tile][whole tiles][head of a tile]; the
        // workgroup holding K step 0 of a tile owns it.  A tail (kt_beg > 0) is always the FIRST segment of its
        // workgroup: it is parked in that workgroup's slot of the workspace (accumulator-register layout, coalesced)
        // and published through a flag, before the workgroup can wait for anything -- so owners only ever wait for
        // work that is never itself blocked.  The owner adds the parked parts of the workgroups after it and writes
        // the finished tile (+ bias) directly.
        unsigned *flags = sk_flags;       // library-owned, all zero between launches (each flag is cleared by its consumer)
        float *slots = Oacc;
        constexpr int SLOT = BM * BN;
        // Slots are written and read 16 bytes per lane with sc1 buffer accesses: a dword sc1 store is one fabric write each
        // (~6x the time per byte of a dwordx4 one), and the 22..54 MB of parked partials per launch were a fifth of the
        // long-reduction launches.  Slot image = accumulator registers in groups of four: [group][lane][4].
        const __amdgpu_buffer_rsrc_t rsrcS = __builtin_amdgcn_make_buffer_rsrc(slots, 0, (unsigned)((size_t)gridDim.x * SLOT * sizeof(float)), 0x00020000);
        typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
        const unsigned slot_lane = (unsigned)(((size_t)wave * (TM * TN * 16 * 64) + (size_t)lane * 4) * sizeof(float));
        if (kt_beg > 0) {
            const unsigned mine = (unsigned)((size_t)wx * SLOT * sizeof(float)) + slot_lane;
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
#pragma unroll
                    for (int q4 = 0; q4 < 4; ++q4) {
                        const f32x4 v = {acc[i][j][4 * q4], acc[i][j][4 * q4 + 1], acc[i][j][4 * q4 + 2], acc[i][j][4 * q4 + 3]};
                        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), rsrcS, mine + ((i * TN + j) * 4 + q4) * 1024, 0, 16);
                    }
            // Agent-scope write-through accesses (sc1: written through / read past the non-coherent per-XCD L2) instead of
            // release/acquire fences: an agent-scope fence writes back and invalidates the whole XCD L2, which evicts the
            // filter slabs and input tiles every other workgroup of the XCD is streaming (measured: +100 us per launch).
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // this wave's slot stores have been acknowledged
            __syncthreads();
            if (tid == 0) __hip_atomic_store(flags + wx, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            continue;
        }
        if (kt_end < nk) {
            const long tile_end = su - kt_end + nk;       // su was already advanced past this segment
            const int G = gridDim.x;
            long covered = su;
            // (deterministic mode relies on this: the parked parts are added in partner-index order p = wx + 1, wx + 2, ... whatever order
            // their flags went up in, and the partition is a function of the shape and the grid alone -- the tile's sum has one fixed order)
            for (int p = wx + 1; covered < tile_end; ++p) {
                if (tid == 0) y2_sk_wait_and_clear(flags, p);      // (bounded: conv_shared.h)
                __syncthreads();
                const unsigned theirs = (unsigned)((size_t)p * SLOT * sizeof(float)) + slot_lane;
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j)
#pragma unroll
                        for (int q4 = 0; q4 < 4; ++q4) {
                            const f32x4 v = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrcS, theirs + ((i * TN + j) * 4 + q4) * 1024, 0, 16));
                            acc[i][j][4 * q4] += v[0];
                            acc[i][j][4 * q4 + 1] += v[1];
                            acc[i][j][4 * q4 + 2] += v[2];
                            acc[i][j][4 * q4 + 3] += v[3];
                        }
                covered = (long)(p + 1) * su_total / G;
            }
        }
    }
    // epilogue: C/D layout of the 32x32 MFMA: col = lane&31, row = (r&3) + 8*(r>>2) + 4*(lane>>5)
    // With bn_part != NULL (forward of a batch-normalised layer) the tile also contributes its columns' shifted sums
    // sum(y - shift), sum((y - shift)^2) of the STORED (rounded) outputs to one of Y2_BN_PART_ROWS partial rows: the
    // statistics pass over y (a full re-read of every activation, 21 launches per step) is gone.
    const bool stats = !BNBWD && SPLITK != 1 && bn_part != nullptr;
    const bool bstats = BNBWD && SPLITK != 1 && bn_part != nullptr;      // (host: only with the wide-store epilogue below)
    // The partial rows are indexed by (pixel tile, wave row); plain stores when the host found a row for every pair (conv_epilogue.h Y2PartRows)
    const Y2PartRows part_rows = Y2PartRows::of(bn_part, Nf, bz.stat_mask_inv);
    auto write_tile = [&](auto checked_tag) {      // interior tiles skip the per-element row test (one VALU compare + branch each)
        constexpr bool CHECKED = decltype(checked_tag)::value;
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int n = n0 + (wn * TN + j) * 32 + (lane & 31);
            if (n >= Nf) continue;
            const float bv = (SPLITK != 1 && bias) ? bias[n] : 0.f;
            const float sh = stats ? bn_shift[n] : 0.f;
            float s1 = 0.f, s2 = 0.f;
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                const int mb = m0 + (wm * TM + i) * 32 + 4 * (lane >> 5);
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int m = mb + (r & 3) + 8 * (r >> 2);
                    if (!CHECKED || m < M) {
                        if (SPLITK == 1) unsafeAtomicAdd(Oacc + (long)m * Nf + n, acc[i][j][r]);
                        else {
                            float v = acc[i][j][r] + bv;
                            if (act_alpha != 1.0f) v = fmaxf(v, act_alpha * v);      // leaky ReLU of a BN-folded inference layer
                            const T o = (T)v;
                            O[(long)m * ldo + n] = o;
                            const float d = (float)o - sh;
                            s1 += d;
                            s2 += d * d;
                        }
                    }
                }
            }
            if (stats) {      // lanes l and l^32 hold the same column (both pass the n < Nf test together)
                s1 += __shfl_xor(s1, 32, 64);
                s2 += __shfl_xor(s2, 32, 64);
                if (lane < 32) part_rows.publish(mt * Plan::STAT_ROWS_FWD + wm, n, s1, s2);
            }
        }
    };
    // Wide-store epilogue.  The accumulator layout puts ONE output element per lane per register: storing straight from it is
    // 16*TM*TN two-byte stores per lane, and the store queue, not HBM, bounded the short-reduction layers (a 128x128x576 tile is
    // 4.6k MFMA cycles; its 32 narrow store instructions per wave took longer than that).  Instead each wave rounds its
    // sub-tile into a private, padded LDS image (the DMA ring is idle by now), computes the statistics from the rounded values
    // on the way, and reads it back row-major: 16 bytes (8 bf16 / 4 f32 consecutive filters of one pixel) per lane per store.
    {
    constexpr int WROWS = Plan::WROWS, WSTRIDE = Plan::WSTRIDE, WCPR = Plan::WCPR;
    constexpr bool WIDE_FITS = SPLITK != 1 && Plan::WIDE_FITS;
    if (WIDE_FITS && wide_store) {
        // producer-layer operands of the fused BN-backward sums: this lane's VEC per-channel constants and the y vectors of the NIT
        // (pixel, chunk) positions it stores below -- all issued back to back, consumed after the staging loop (one exposed latency per
        // tile instead of one per store).  Stream-K workgroups (256 VGPRs per wave) issue them ahead of the staging loop.
        constexpr int NIT = WROWS * WCPR / 64;
        constexpr int YG = NIT < 4 ? NIT : 4;       // y vectors in flight per lane (the 256-pixel tile spills with all 8)
        constexpr bool BZ_EARLY = SPLITK == 2 && BM == 128;
        Y2BnBwdLane<T> bw;
        Vec16<T> yv[YG];
        const int bz_nb = min(n0 + wn * TN * 32 + (lane % WCPR) * VEC, Nf - VEC);      // (clamped: out-of-range chunks are never summed)
        auto bz_load_y = [&](int it0) {
#pragma unroll
            for (int u = 0; u < YG; ++u) {
                const int m = min(m0 + wm * WROWS + ((it0 + u) * 64 + lane) / WCPR, M - 1);
                yv[u] = ld16(reinterpret_cast<const T *>(bz.Y) + (long)m * Nf + bz_nb);
            }
        };
        auto bz_prefetch = [&]() {
            bz_load_y(0);
            bw.load(bz, bz_nb);
        };
        if (bstats && BZ_EARLY) bz_prefetch();
        __syncthreads();                       // every wave has finished reading the last K step's stage
        unsigned char *wreg = smem + wave * (WROWS * WSTRIDE);
        const bool tail = m0 + BM > M;
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int n = n0 + (wn * TN + j) * 32 + (lane & 31);
            const bool n_ok = n < Nf;
            const float bv = (bias && n_ok) ? bias[n] : 0.f;
            const float sh = (stats && n_ok) ? bn_shift[n] : 0.f;
            float s1 = 0.f, s2 = 0.f;
#pragma unroll
            for (int i = 0; i < TM; ++i) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = i * 32 + 4 * (lane >> 5) + (r & 3) + 8 * (r >> 2);
                    float v = acc[i][j][r] + bv;
                    if (act_alpha != 1.0f) v = fmaxf(v, act_alpha * v);
                    const T o = (T)v;
                    *reinterpret_cast<T *>(wreg + row * WSTRIDE + (j * 32 + (lane & 31)) * (int)sizeof(T)) = o;
                    if (stats && (!tail || m0 + wm * WROWS + row < M)) {
                        const float d = (float)o - sh;
                        s1 += d;
                        s2 += d * d;
                    }
                }
            }
            if (stats) {
                s1 += __shfl_xor(s1, 32, 64);
                s2 += __shfl_xor(s2, 32, 64);
                if (lane < 32 && n_ok) part_rows.publish(mt * Plan::STAT_ROWS_FWD + wm, n, s1, s2);
            }
        }
        // (LDS operations of one wave execute in order: its own reads below see its own writes above)
        // BN + leaky backward sums of the producer layer (bz): a lane keeps the same VEC filters in every iteration (64 % WCPR == 0)
        static_assert(64 % WCPR == 0, "a lane stays on one column chunk");
        if (bstats && !BZ_EARLY) bz_prefetch();
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            y2_store_chunk<WSTRIDE, WCPR>(wreg, it * 64 + lane, 0, O, ldo, m0 + wm * WROWS, M, n0 + wn * TN * 32, Nf, bstats, bw, bz, yv[it % YG],
                                          [&] { if (bstats && it && it % YG == 0) bz_load_y(it); });      // (the next YG y vectors, behind this LDS read)
        }
        if (bstats) {
            bw.template lane_group_sum<WCPR>();
            // Where the LDS plan leaves room behind the tile images the WGM wave rows meet there and the tile leaves ONE partial row per filter
            // (Plan::STAT_ROWS_BNBWD: what the host counts)
            constexpr bool RED = BNBWD && Plan::RED;
            static_assert(!BNBWD || Plan::STAT_ROWS_BNBWD == (RED ? 1 : WGM), "the host counts the rows this epilogue writes");
            const int nb = n0 + wn * TN * 32 + lane * VEC;
            bool writer = lane < WCPR && nb < Nf;
            if constexpr (RED) {
                writer = writer && wm == 0;
                y2_wave_rows_meet<WGM, WGN, WCPR>(reinterpret_cast<float *>(smem + Plan::IMAGES), wave, wn, lane, writer, bw.ps);
            }
            if (writer) part_rows.publish(mt * Plan::STAT_ROWS_BNBWD + (RED ? 0 : wm), nb, bw.ps);
        }
    } else if (m0 + BM <= M) write_tile(std::false_type{});
    else write_tile(std::true_type{});
    }
    if (SPLITK != 2) break;
  }
}

// f32 partial sums [M][Nf] -> O (dtype, pixel stride ldo) + bias
template <typename T>
__global__ void splitk_finish_kernel(const float *__restrict__ acc, const float *__restrict__ bias, T *__restrict__ O, long M, int Nf, int ldo, float act_alpha) {
    const long total = M * Nf;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long m = i / Nf;
        const int n = (int)(i - m * Nf);
        float v = acc[i] + (bias ? bias[n] : 0.f);
        if (act_alpha != 1.0f) v = fmaxf(v, act_alpha * v);
        O[m * ldo + n] = (T)v;
    }
}

// Stream-K hand-off flags: Y2_STREAM_FLAG_SETS sets of Y2_STREAM_FLAG_WORDS words per device, allocated and zeroed once; a
// launch takes the next set round-robin (launches on different streams may overlap) and leaves it zero (every flag is
// cleared by the one workgroup that waits for it), so no per-launch memset node is needed (16 of them cost 83 us a step).
#define Y2_STREAM_FLAG_SETS 8
// The ONE piece of library-owned device state (declared in include/yolo2_hip.h): 32 KiB per device, created on first use
// under a mutex, handed out round-robin under the same mutex (host threads may launch concurrently), freed by yolo2_shutdown().
static std::mutex g_flag_mutex;
static unsigned *g_flag_pool[64] = {nullptr};
static unsigned g_flag_counter[64] = {0};
static std::atomic<unsigned> g_sk_wait_ticks{0};       // 0 = Y2_SK_DEFAULT_WAIT_TICKS (tests shorten it: yolo2_debug_set_streamk_wait_us)
static std::atomic<int> g_sk_unclamped{0};             // tests only: lets a forced grid exceed the number of K steps (the partition bug the wait bound exists for)
int y2_sk_unclamped() { return g_sk_unclamped.load(std::memory_order_relaxed); }
__global__ void async_error_gather_kernel(const unsigned *__restrict__ pool, unsigned *__restrict__ host_words) {
    if (threadIdx.x < Y2_STREAM_FLAG_SETS)
        host_words[threadIdx.x] = __hip_atomic_load(pool + (size_t)threadIdx.x * Y2_STREAM_FLAG_STRIDE + Y2_STREAM_FLAG_WORDS, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// the current device's pool, created on first use (caller holds g_flag_mutex); does NOT advance the rotating set counter
static unsigned *ensure_pool_locked(int dev) {
    if (!g_flag_pool[dev]) {
        unsigned *p = nullptr;
        const size_t bytes = (size_t)Y2_STREAM_FLAG_SETS * Y2_STREAM_FLAG_STRIDE * sizeof(unsigned);
        if (hipMalloc((void **)&p, bytes) != hipSuccess) return nullptr;
        if (hipMemset(p, 0, bytes) != hipSuccess || hipDeviceSynchronize() != hipSuccess) { (void)hipFree(p); return nullptr; }
        g_flag_pool[dev] = p;
    }
    return g_flag_pool[dev];
}
unsigned *y2_stream_flags() {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
    std::lock_guard<std::mutex> lock(g_flag_mutex);
    unsigned *pool = ensure_pool_locked(dev);
    if (!pool) return nullptr;
    return pool + (size_t)(g_flag_counter[dev]++ % Y2_STREAM_FLAG_SETS) * Y2_STREAM_FLAG_STRIDE;
}
// Enqueues, on `stream`, a copy of the CURRENT device's give-up counters (one word per flag set) into caller-owned pinned host memory: the
// asynchronous form of yolo2_check_async_errors.  A host that finds a non-zero word once the copy has completed (event / stream query) calls
// yolo2_check_async_errors, which reports and re-zeroes the pool.  Costs one 32-byte device-to-host copy; nothing is synchronised.
extern "C" int yolo2_async_error_snapshot(unsigned *host_words, void *stream) {
    if (!host_words) { yolo2_set_error("yolo2_async_error_snapshot: host_words is NULL"); return YOLO2_E_ARG; }
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) { yolo2_set_error("yolo2_async_error_snapshot: no current device"); return YOLO2_E_LAUNCH; }
    unsigned *pool;
    {
        std::lock_guard<std::mutex> lock(g_flag_mutex);
        pool = g_flag_pool[dev];
    }
    if (!pool) {      // no stream-K launch has run on this device yet: nothing can have given up
        for (int i = 0; i < YOLO2_ASYNC_ERROR_WORDS; ++i) host_words[i] = 0u;
        return YOLO2_OK;
    }
    static_assert(YOLO2_ASYNC_ERROR_WORDS == Y2_STREAM_FLAG_SETS, "one status word per flag set");
    // one eight-lane kernel writing straight into the pinned (device-mapped) host words: a strided 2-D copy of eight words goes through the runtime's
    // staging path and costs tens of microseconds of stream time (measured: +0.4 % on the training step when enqueued every eighth step)
    async_error_gather_kernel<<<1, 64, 0, (hipStream_t)stream>>>(pool, host_words);
    Y2_CHECK_LAUNCH();
    return YOLO2_OK;
}
// Synchronises `stream` and reports what only the device can know: a stream-K owner that gave up waiting for a partner's partial tile
// (y2_sk_wait_and_clear).  The pool is re-zeroed so that the process can go on, but every result since the previous check is suspect.
// Per device: reads and resets the pool of the CURRENT device only (a process driving several devices checks each under hipSetDevice).
extern "C" int yolo2_check_async_errors(void *stream) {
    int dev = 0;
    if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess || hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) {
        yolo2_set_error("yolo2_check_async_errors: HIP error: %s", hipGetErrorString(hipGetLastError()));
        return YOLO2_E_LAUNCH;
    }
    std::lock_guard<std::mutex> lock(g_flag_mutex);
    if (!g_flag_pool[dev]) return YOLO2_OK;
    unsigned status[Y2_STREAM_FLAG_SETS] = {0};
    if (hipMemcpy2D(status, sizeof(unsigned), g_flag_pool[dev] + Y2_STREAM_FLAG_WORDS, Y2_STREAM_FLAG_STRIDE * sizeof(unsigned), sizeof(unsigned),
                    Y2_STREAM_FLAG_SETS, hipMemcpyDeviceToHost) != hipSuccess) {
        yolo2_set_error("yolo2_check_async_errors: reading the stream-K status words failed");
        return YOLO2_E_LAUNCH;
    }
    unsigned gave_up = 0;
    for (int i = 0; i < Y2_STREAM_FLAG_SETS; ++i) gave_up += status[i];
    if (!gave_up) return YOLO2_OK;
    (void)hipDeviceSynchronize();
    (void)hipMemset(g_flag_pool[dev], 0, (size_t)Y2_STREAM_FLAG_SETS * Y2_STREAM_FLAG_STRIDE * sizeof(unsigned));
    const unsigned ticks = g_sk_wait_ticks.load(std::memory_order_relaxed);
    for (int i = 0; ticks && i < Y2_STREAM_FLAG_SETS; ++i)
        (void)hipMemcpy(g_flag_pool[dev] + (size_t)i * Y2_STREAM_FLAG_STRIDE + Y2_STREAM_FLAG_WORDS + 1, &ticks, sizeof(ticks), hipMemcpyHostToDevice);
    yolo2_set_error("stream-K hand-off: %u wait(s) for a partner workgroup's partial tile gave up; convolution outputs since the last check are invalid", gave_up);
    return YOLO2_E_LAUNCH;
}
// tests: wait limit of the stream-K owners in microseconds (0 = default, 2 s) and the grid clamp (unclamped != 0 lets yolo2_debug_set_pp force
// more workgroups than K steps -- an unserviceable partition)
extern "C" int yolo2_debug_set_streamk_wait_us(int us, int unclamped) {
    if (us < 0 || (unsigned)us > 0xffffffffu / 100u) { yolo2_set_error("yolo2_debug_set_streamk_wait_us: us outside 0 .. %u (100 MHz ticks in 32 bits)", 0xffffffffu / 100u); return YOLO2_E_ARG; }
    const unsigned ticks = (unsigned)us * 100u;
    g_sk_wait_ticks.store(ticks, std::memory_order_relaxed);
    g_sk_unclamped.store(unclamped, std::memory_order_relaxed);
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) { yolo2_set_error("yolo2_debug_set_streamk_wait_us: no current device"); return YOLO2_E_LAUNCH; }
    std::lock_guard<std::mutex> lock(g_flag_mutex);
    if (!ensure_pool_locked(dev)) { yolo2_set_error("yolo2_debug_set_streamk_wait_us: no flag pool"); return YOLO2_E_LAUNCH; }
    (void)hipDeviceSynchronize();
    for (int i = 0; i < Y2_STREAM_FLAG_SETS; ++i)
        if (hipMemcpy(g_flag_pool[dev] + (size_t)i * Y2_STREAM_FLAG_STRIDE + Y2_STREAM_FLAG_WORDS + 1, &ticks, sizeof(ticks), hipMemcpyHostToDevice) != hipSuccess)
            return YOLO2_E_LAUNCH;
    return YOLO2_OK;
}
extern "C" int yolo2_shutdown(void) {
    std::lock_guard<std::mutex> lock(g_flag_mutex);
    int cur = 0;
    (void)hipGetDevice(&cur);
    for (int d = 0; d < 64; ++d)
        if (g_flag_pool[d]) {
            if (hipSetDevice(d) == hipSuccess) { (void)hipDeviceSynchronize(); (void)hipFree(g_flag_pool[d]); }
            g_flag_pool[d] = nullptr;
            g_flag_counter[d] = 0;
        }
    (void)hipSetDevice(cur);
    return YOLO2_OK;
}

// The lines of conv_igemm_table.h.  Which line a shape gets is conv_route.hip's business (y2_conv_route).
template <typename T, int BM, int BN, int WGN, int NS, int KS, int SPLIT, bool CT, int CH, int NW, bool BW>
static void igemm_launch(int grid_x, int grid_y, const Y2IgemmArgs &a, hipStream_t st) {
    static_assert(!BW || (Y2IgemmPlan<T, BM, BN, WGN, NS, CH, NW>::WIDE_FITS && SPLIT != 1 && !CT), "a BN-backward line no route can name");
    conv_igemm_kernel<T, BN, WGN, NS, KS, SPLIT, CT, CH, NW, BM, BW><<<dim3(grid_x, grid_y), NW * 64, 0, st>>>(
        (const T *)a.P, a.p_bytes, (const T *)a.F, a.f_bytes, a.bias, (T *)a.O, a.ws, a.H, a.W, a.Cp, a.ldp, a.Nf, a.ldo, a.M, a.NT, a.remap, a.bn_shift,
        a.bn_part, a.sk_flags, a.act_alpha, a.wide_store, a.bz);
}
#define Y2_LINE(T, DT, BM, BN, WGN, NS, KS, SPLIT, CT, CH, NW, BW)                                                                        \
    {{DT, BM, BN, WGN, NS, KS, SPLIT, CT, CH, NW, BW}, Y2IgemmPlan<T, BM, BN, WGN, NS, CH, NW>::WIDE_FITS, Y2IgemmPlan<T, BM, BN, WGN, NS, CH, NW>::STAT_ROWS_FWD, \
     Y2IgemmPlan<T, BM, BN, WGN, NS, CH, NW>::STAT_ROWS_BNBWD, igemm_launch<T, BM, BN, WGN, NS, KS, SPLIT, CT != 0, CH, NW, BW != 0>},
#define Y2_F32(...) Y2_LINE(float, YOLO2_F32, __VA_ARGS__)
#define Y2_BF16(...) Y2_LINE(bf16, YOLO2_BF16, __VA_ARGS__)
#define Y2_TWIN_NONE(...)
#define Y2_TWIN_BF16(...) Y2_BF16(__VA_ARGS__, 1)
#define Y2_TWIN_BOTH(...) Y2_F32(__VA_ARGS__, 1) Y2_BF16(__VA_ARGS__, 1)
#define Y2_KS(BM, BN, WGN, NS, KS, SPLIT, CT, CH, NW, TW) Y2_F32(BM, BN, WGN, NS, KS, SPLIT, CT, CH, NW, 0) Y2_BF16(BM, BN, WGN, NS, KS, SPLIT, CT, CH, NW, 0) Y2_TWIN_##TW(BM, BN, WGN, NS, KS, SPLIT, CT, CH, NW)
#define Y2_ROW_K3(BM, BN, WGN, NS, ...) Y2_KS(BM, BN, WGN, NS, 3, __VA_ARGS__)
#define Y2_ROW_K31(BM, BN, WGN, NS, ...) Y2_KS(BM, BN, WGN, NS, 3, __VA_ARGS__) Y2_KS(BM, BN, WGN, NS, 1, __VA_ARGS__)
#define Y2_ROW(BM, BN, WGN, NS, SPLIT, CT, CH, NW, KSET, TW) Y2_ROW_##KSET(BM, BN, WGN, NS, SPLIT, CT, CH, NW, TW)
static const Y2IgemmLine g_igemm_lines[] = {Y2_IGEMM_TABLE(Y2_ROW)};
const Y2IgemmLine *y2_igemm_line(const Y2IgemmKey &key) {
    for (const Y2IgemmLine &l : g_igemm_lines)
        if (!memcmp(&l.key, &key, sizeof(key))) return &l;
    return nullptr;
}
void y2_splitk_finish(const float *acc, const float *bias, void *O, long M, int Nf, int ldo, float act_alpha, int dtype, hipStream_t st) {
    const long total = M * Nf;
    const int g = (int)((total + 255) / 256 < 2048 ? (total + 255) / 256 : 2048);
    if (dtype == YOLO2_BF16) splitk_finish_kernel<bf16><<<g, 256, 0, st>>>(acc, bias, (bf16 *)O, M, Nf, ldo, act_alpha);
    else splitk_finish_kernel<float><<<g, 256, 0, st>>>(acc, bias, (float *)O, M, Nf, ldo, act_alpha);
}
