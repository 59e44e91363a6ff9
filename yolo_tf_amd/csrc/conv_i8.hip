// NHWC implicit-GEMM convolution on the int8 MFMA (gfx950): the quantised inference path.
//
//   acc[m, n] = sum_{tap, c} P[pix(m) + shift(tap), c] * F[n][tap*Cp + c]          exact int32
//   t = float(acc) * mult[n];  y = t + bias[n];  y = y > 0 ? y : y * alpha         f32, two roundings (built with -ffp-contract=off)
//   O = int8 clip(rint(y * inv_s_out)) | bf16(y) | f32 y | the raw int32 acc       (out_kind)
//
// Structure: conv_igemm.hip's, restated for bytes.  One workgroup = 4 waves (2 x 2) = a 128-pixel x BN-filter tile; a K step is 64 channels
// of one tap (a 64-byte row = four 16-byte chunks).  Operands go to LDS by DMA (buffer_load_dwordx4 ... lds) with the XOR swizzle applied on
// the source side; SAME padding, the pixel tail, the filter tail and the channel tail (Cp is a multiple of 16, not of 64) are out-of-range
// buffer offsets, which the DMA turns into zeros.  Two LDS stages: the DMA of step t+1 is issued right after the barrier of step t and
// overlaps its MFMAs.  A = pixels, B = filters on v_mfma_i32_32x32x32_i8: lane l holds the 16 bytes k = 16*(l>>5) .. +15 of row / column l&31
// -- the byte image of the bf16 32x32x16 operand -- and the C/D layout is the dtype-independent one (col = l&31,
// row = (r&3) + 8*(r>>2) + 4*(l>>5)); tests/test_quant_gpu.py pins both with exact integer data against an int64 NumPy convolution.
// The filter operand is [Nf][tap][Cp] int8, prepared on the host once per checkpoint (yolo_tf_amd/quant.py).
// Not here yet: stream-K / K slicing for the under-filled 13x13 grids, a wide-store epilogue, a fused pool.
#include "common.h"

typedef __attribute__((ext_vector_type(4))) int i32x4;
typedef __attribute__((ext_vector_type(16))) int i32x16;

#define I8_OOB 0x80000000u      // any offset >= num_records makes the buffer DMA return zeros

template <int BN, int KS>
__global__ __launch_bounds__(256) void conv_i8_kernel(const int8_t *__restrict__ P, unsigned p_bytes, const int8_t *__restrict__ F, unsigned f_bytes,
                                                      const float *__restrict__ mult, const float *__restrict__ bias, void *__restrict__ O, int H, int W,
                                                      int Cp, int ldp, int Nf, int ldo, int M, int NT, float alpha, float inv_s_out, int out_kind) {
    constexpr int BM = 128, NW = 4, WGN = 2, TM = 2, TN = BN / 64;
    constexpr int TAPS = KS * KS, PAD = KS / 2;
    constexpr int ROWB = 64, CH = 4, BK = 64;      // bytes (= channels) per tile row and K step
    constexpr int RPL = 256 / ROWB;                // rows per 256-byte LDS bank line
    constexpr int RPI = 1024 / ROWB;               // rows per DMA instruction (1 KiB)
    constexpr int A_IT = BM / RPI / NW;
    constexpr int B_PIECES = BN / RPI;
    constexpr int B_IT = (B_PIECES + NW - 1) / NW;
    constexpr int STAGE = (BM + BN) * ROWB;
    static_assert(TN >= 1 && A_IT >= 1 && B_IT >= 1, "tile");

    __shared__ __attribute__((aligned(1024))) unsigned char smem[2 * STAGE];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WGN, wn = wave % WGN;
    const int nt = blockIdx.x % NT, mt = blockIdx.x / NT;
    const int m0 = mt * BM, n0 = nt * BN;
    const int kpc = (Cp + BK - 1) / BK;            // K steps per tap
    const int nk = TAPS * kpc;

    const __amdgpu_buffer_rsrc_t rsrcP = __builtin_amdgcn_make_buffer_rsrc(const_cast<int8_t *>(P), 0, p_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rsrcF = __builtin_amdgcn_make_buffer_rsrc(const_cast<int8_t *>(F), 0, f_bytes, 0x00020000);
    const int lrow = lane / CH, lslot = lane % CH;

    // per-lane source descriptors: byte offset of (row, swizzled chunk) and the set of taps inside the image
    unsigned a_voff[A_IT], a_mask[A_IT], a_cb[A_IT];
#pragma unroll
    for (int i = 0; i < A_IT; ++i) {
        const int r = (wave * A_IT + i) * RPI + lrow;
        a_cb[i] = (unsigned)((lslot ^ ((r / RPL) % CH)) * 16);
        const int m = m0 + r;
        unsigned mask = 0;
        if (m < M) {
            const int rem = m % (H * W);
            const int h = rem / W, w = rem - h * W;
            if (KS == 3) {
                const unsigned cm = (w > 0 ? 1u : 0u) | 2u | (w < W - 1 ? 4u : 0u);
                mask = (h > 0 ? cm : 0u) | (cm << 3) | (h < H - 1 ? cm << 6 : 0u);
            } else {
                mask = 1u;
            }
        }
        a_mask[i] = mask;
        a_voff[i] = (unsigned)m * (unsigned)ldp + a_cb[i];
    }
    unsigned b_voff[B_IT], b_cb[B_IT];
#pragma unroll
    for (int i = 0; i < B_IT; ++i) {
        const int piece = wave * B_IT + i;
        const int r = piece * RPI + lrow;
        b_cb[i] = (unsigned)((lslot ^ ((r / RPL) % CH)) * 16);
        const int n = n0 + r;
        const bool ok = piece < B_PIECES && n < Nf;
        b_voff[i] = ok ? (unsigned)n * (unsigned)(TAPS * Cp) + b_cb[i] : I8_OOB;
    }

    i32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0;

    // issue cursor (wave-uniform scalars), one step ahead of the compute cursor
    int kt_issue = 0, i_tap = 0, i_c0 = 0, i_dh = -PAD, i_dw = -PAD, i_stage = 0;
    auto issue_next = [&]() {
        const unsigned tapbit = 1u << i_tap;
        const unsigned offA = (unsigned)((i_dh * W + i_dw) * ldp + i_c0);      // may wrap: added mod 2^32
        const unsigned offB = (unsigned)(i_tap * Cp + i_c0);
        unsigned char *As = smem + i_stage * STAGE;
        unsigned char *Bs = As + BM * ROWB;
#pragma unroll
        for (int i = 0; i < A_IT; ++i) {
            const bool ok = (a_mask[i] & tapbit) != 0 && (unsigned)i_c0 + a_cb[i] < (unsigned)Cp;
            const unsigned voff = ok ? a_voff[i] + offA : I8_OOB;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrcP, (__attribute__((address_space(3))) void *)(As + (wave * A_IT + i) * 1024), 16, voff, 0, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < B_IT; ++i) {
            if (wave * B_IT + i < B_PIECES) {      // (wave-uniform: with BN = 64 every wave owns exactly one piece)
                const bool ok = b_voff[i] != I8_OOB && (unsigned)i_c0 + b_cb[i] < (unsigned)Cp;
                const unsigned voff = ok ? b_voff[i] + offB : I8_OOB;
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrcF, (__attribute__((address_space(3))) void *)(Bs + (wave * B_IT + i) * 1024), 16, voff, 0, 0, 0);
            }
        }
        ++kt_issue;
        i_stage ^= 1;
        i_c0 += BK;
        if (i_c0 >= Cp) {
            i_c0 = 0;
            ++i_tap;
            if (++i_dw > PAD) { i_dw = -PAD; ++i_dh; }
        }
    };
    issue_next();

    const int frow = lane & 31;
    const int fsw = (frow / RPL) % CH;
    int c_stage = 0;
    for (int kt = 0; kt < nk; ++kt) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // this wave's pieces of step kt have landed
        __builtin_amdgcn_s_barrier();                          // ... and every wave's; step kt-1's stage is free
        if (kt_issue < nk) issue_next();
        const unsigned char *As = smem + c_stage * STAGE + (wm * TM * 32 + frow) * ROWB;
        const unsigned char *Bs = smem + c_stage * STAGE + (BM + wn * TN * 32 + frow) * ROWB;
        c_stage ^= 1;
#pragma unroll
        for (int kk = 0; kk < BK / 32; ++kk) {
            const int boff = ((kk * 2 + (lane >> 5)) ^ fsw) * 16;      // the 16-byte chunk holding this lane's 16 k values
            i32x4 af[TM], bf[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) af[i] = *reinterpret_cast<const i32x4 *>(As + i * 32 * ROWB + boff);
#pragma unroll
            for (int j = 0; j < TN; ++j) bf[j] = *reinterpret_cast<const i32x4 *>(Bs + j * 32 * ROWB + boff);
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(af[i], bf[j], acc[i][j], 0, 0, 0);
        }
    }

    // epilogue: col = lane&31, row = (r&3) + 8*(r>>2) + 4*(lane>>5); every store is bounds-checked (m < M, n < Nf)
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int n = n0 + (wn * TN + j) * 32 + (lane & 31);
        if (n >= Nf) continue;
        const float mu = out_kind != YOLO2_I8_OUT_ACC ? mult[n] : 0.f;
        const float bv = out_kind != YOLO2_I8_OUT_ACC ? bias[n] : 0.f;
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const int mb = m0 + (wm * TM + i) * 32 + 4 * (lane >> 5);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = mb + (r & 3) + 8 * (r >> 2);
                if (m >= M) continue;
                const long o = (long)m * ldo + n;
                const int a = acc[i][j][r];
                if (out_kind == YOLO2_I8_OUT_ACC) {
                    reinterpret_cast<int *>(O)[o] = a;
                    continue;
                }
                const float t = (float)a * mu;
                float y = t + bv;
                if (alpha != 1.0f) y = y > 0.f ? y : y * alpha;
                if (out_kind == YOLO2_I8_OUT_I8) {
                    float q = rintf(y * inv_s_out);
                    q = q != q ? 0.f : fminf(fmaxf(q, -127.f), 127.f);
                    reinterpret_cast<int8_t *>(O)[o] = (int8_t)(int)q;
                } else if (out_kind == YOLO2_I8_OUT_BF16) {
                    reinterpret_cast<bf16 *>(O)[o] = (bf16)y;
                } else {
                    reinterpret_cast<float *>(O)[o] = y;
                }
            }
        }
    }
}

extern "C" int yolo2_conv2d_i8(const void *P, const void *F, const float *mult, const float *bias, void *O, int B, int H, int W, int Cp, int ldp,
                               int Nf, int ldo, int ksize, float alpha, float inv_s_out, int out_kind, void *stream) {
    Y2_CHECK_ARG(P && F && O);
    Y2_CHECK_ARG(out_kind >= YOLO2_I8_OUT_I8 && out_kind <= YOLO2_I8_OUT_ACC);
    Y2_CHECK_ARG(out_kind == YOLO2_I8_OUT_ACC || (mult && bias));
    Y2_CHECK_ARG(B > 0 && H > 0 && W > 0 && Nf > 0);
    Y2_CHECK_ARG(ksize == 1 || ksize == 3);
    Y2_CHECK_ARG(Cp > 0 && Cp % 16 == 0);                     // a pixel's channels are whole 16-byte DMA chunks
    Y2_CHECK_ARG(ldp >= Cp && ldp % 16 == 0 && ldo >= Nf);
    Y2_CHECK_ARG(((uintptr_t)P & 15) == 0 && ((uintptr_t)F & 15) == 0);
    const int osize = out_kind == YOLO2_I8_OUT_I8 ? 1 : out_kind == YOLO2_I8_OUT_BF16 ? 2 : 4;
    Y2_CHECK_ARG(((uintptr_t)O & (uintptr_t)(osize - 1)) == 0);
    const long M = (long)B * H * W;
    const long p_bytes = (M - 1) * ldp + Cp, f_bytes = (long)Nf * ksize * ksize * Cp;
    Y2_CHECK_ARG(M < (1L << 31) - 128 && p_bytes < (1L << 31) && f_bytes < (1L << 31));      // 32-bit buffer offsets below the out-of-range marker
    // the largest |acc| is ksize^2 * Cp * 128 * 128 (a -128 against a -128): int32 holds it for every Cp this check lets through
    Y2_CHECK_ARG((long)ksize * ksize * Cp <= (1L << 31) / (128 * 128) - 1);
    const int MT = cdiv(M, 128);
    hipStream_t st = (hipStream_t)stream;
#define Y2_I8_LAUNCH(BN_, KS_)                                                                                                                  \
    do {                                                                                                                                        \
        const int NT = cdiv(Nf, BN_);                                                                                                           \
        Y2_CHECK_ARG((long)MT * NT < (1L << 31));                                                                                               \
        conv_i8_kernel<BN_, KS_><<<dim3((unsigned)(MT * NT)), dim3(256), 0, st>>>((const int8_t *)P, (unsigned)p_bytes, (const int8_t *)F,     \
            (unsigned)f_bytes, mult, bias, O, H, W, Cp, ldp, Nf, ldo, (int)M, NT, alpha, inv_s_out, out_kind);                                  \
    } while (0)
    if (Nf <= 64) {
        if (ksize == 3) Y2_I8_LAUNCH(64, 3); else Y2_I8_LAUNCH(64, 1);
    } else {
        if (ksize == 3) Y2_I8_LAUNCH(128, 3); else Y2_I8_LAUNCH(128, 1);
    }
#undef Y2_I8_LAUNCH
    Y2_CHECK_LAUNCH();
    return YOLO2_OK;
}
