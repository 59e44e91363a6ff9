// MFMA operand layouts of the convolution filters (gfx950): per layer, all layers in one launch, and fused with the Adam update of the f32 masters.
#include "common.h"
#include "adam.h"

// ------------------------------------------------------------------------------------------
// filter prep: HWIO f32 -> K-contiguous operand layouts (reference stores conv weights HWIO,
// parse_darknet_yolo2.py:95-97)
// ------------------------------------------------------------------------------------------
template <typename T>
__global__ void filter_fwd_kernel(const float *__restrict__ Wt, T *__restrict__ F, int Cin, int ldcin, int Cout, int taps) {
    __shared__ float tile[32][33];
    const int tap = blockIdx.z;
    const int n0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
    const int tx = threadIdx.x, ty = threadIdx.y;  // 32 x 8
    for (int i = ty; i < 32; i += 8) {
        int c = c0 + i, n = n0 + tx;
        tile[i][tx] = (c < Cin && n < Cout) ? Wt[((long)tap * Cin + c) * Cout + n] : 0.f;
    }
    __syncthreads();
    const long Kf = (long)taps * ldcin;
    for (int i = ty; i < 32; i += 8) {
        int n = n0 + i, c = c0 + tx;
        if (n < Cout && c < ldcin) F[n * Kf + y2_filter_koff(tap, c, ldcin, taps)] = (T)tile[tx][i];
    }
}
template <typename T>
__global__ void filter_dgrad_kernel(const float *__restrict__ Wt, T *__restrict__ F, int Cin, int Cout, int ldcout, int taps) {
    const long total = (long)Cin * taps * ldcout;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        int n = (int)(i % ldcout);
        long r = i / ldcout;
        int tp = (int)(r % taps);
        int c = (int)(r / taps);
        float v = n < Cout ? Wt[((long)(taps - 1 - tp) * Cin + c) * Cout + n] : 0.f;
        F[c * (long)taps * ldcout + y2_filter_koff(tp, n, ldcout, taps)] = (T)v;
    }
}

extern "C" int yolo2_filter_prep(const float *W, void *Ffwd, void *Fdgr, int ksize, int Cin, int ldcin,
                                 int Cout, int ldcout, int dtype, void *stream) {
    Y2_CHECK_ARG(W && (Ffwd || Fdgr));
    Y2_CHECK_ARG(ksize == 1 || ksize == 3);
    Y2_CHECK_ARG(ldcin >= Cin && ldcout >= Cout);
    hipStream_t st = (hipStream_t)stream;
    const int taps = ksize * ksize;
    if (Ffwd) {
        dim3 grid(cdiv(Cout, 32), cdiv(ldcin, 32), taps), block(32, 8);
        Y2_DISPATCH_DTYPE(dtype, filter_fwd_kernel<T><<<grid, block, 0, st>>>(W, (T *)Ffwd, Cin, ldcin, Cout, taps));
    }
    if (Fdgr) {
        long total = (long)Cin * taps * ldcout;
        int grid = (int)(total / 256 + 1 < 4096 ? total / 256 + 1 : 4096);
        Y2_DISPATCH_DTYPE(dtype, filter_dgrad_kernel<T><<<grid, 256, 0, st>>>(W, (T *)Fdgr, Cin, Cout, ldcout, taps));
    }
    Y2_CHECK_LAUNCH();
    return YOLO2_OK;
}

// All layers in ONE launch (the per-layer calls were 43 launches of ~9 us each per training step): a device
// table of descriptors; work unit u of a layer = one 64 x 64 (c, n) tile of one tap, handling BOTH layouts
// from the same LDS tile (Ffwd needs the transpose, Fdgr is a re-strided copy).  16-byte loads and stores
// (a 32 x 32 tile with 2-byte stores ran at 2.5 TB/s: 215 us per training step).
template <typename T>
__device__ __forceinline__ void store8(T *dst, const float (&v)[8]) {
    if constexpr (sizeof(T) == 2) {
        bf16x8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = (bf16)v[j];
        *reinterpret_cast<bf16x8 *>(dst) = o;
    } else {
        f32x4 a = {v[0], v[1], v[2], v[3]}, b = {v[4], v[5], v[6], v[7]};
        reinterpret_cast<f32x4 *>(dst)[0] = a;
        reinterpret_cast<f32x4 *>(dst)[1] = b;
    }
}
// Both operand layouts of one TC x TN (c, n) tile of one tap, from its fresh f32 values in LDS: Ffwd rows n with c contiguous (the transpose),
// Fdgr rows c with n contiguous and the taps flipped.  8 elements (16 bytes of bf16) per lane and store.
template <typename T>
__device__ __forceinline__ void filter_tile_emit(const yolo2_filter_desc &d, const float (&tile)[YOLO2_FILTER_PREP_TILE][YOLO2_FILTER_PREP_TILE_N + 1], int tap, int taps,
                                                 int c0, int n0, int tid) {
    constexpr int TC = YOLO2_FILTER_PREP_TILE, TN = YOLO2_FILTER_PREP_TILE_N;
    T *Ff = (T *)d.Ffwd, *Fd = (T *)d.Fdgr;
    if (Ff) {       // rows n, c contiguous: TC / 8 lanes per row (the tile's odd pitch keeps the transposed reads conflict-free)
        constexpr int LPR = TC / 8, RPP = 256 / LPR;
        const int g8 = (tid % LPR) * 8, rr = tid / LPR;
        const long Kf = (long)taps * d.ldcin;
#pragma unroll
        for (int p = 0; p < TN / RPP; ++p) {
            const int nl = rr + p * RPP, nn = n0 + nl, c = c0 + g8;
            if (nn < d.cout && c < d.ldcin) {
                float v[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) v[j] = tile[g8 + j][nl];
                store8<T>(Ff + nn * Kf + y2_filter_koff(tap, c, d.ldcin, taps), v);
            }
        }
    }
    if (Fd) {       // rows c, n contiguous, taps flipped: TN / 8 lanes per row
        constexpr int LPR = TN / 8, RPP = 256 / LPR;
        const int g8 = (tid % LPR) * 8, rr = tid / LPR;
        const long Kd = (long)taps * d.ldcout;
        const int tp = taps - 1 - tap;
#pragma unroll
        for (int p = 0; p < TC / RPP; ++p) {
            const int cl = rr + p * RPP, c = c0 + cl, nn = n0 + g8;
            if (c < d.cin && nn < d.ldcout) {
                float v[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) v[j] = tile[cl][g8 + j];
                store8<T>(Fd + c * Kd + y2_filter_koff(tp, nn, d.ldcout, taps), v);
            }
        }
    }
}
template <typename T>
__global__ __launch_bounds__(256) void filter_prep_batch_kernel(const yolo2_filter_desc *__restrict__ descs, int n) {
    constexpr int TC = YOLO2_FILTER_PREP_TILE, TN = YOLO2_FILTER_PREP_TILE_N;
    __shared__ float tile[TC][TN + 1];
    int li = 0;
    while (li + 1 < n && (int)blockIdx.x >= descs[li + 1].first_block) ++li;
    const yolo2_filter_desc d = descs[li];
    const int taps = d.ksize * d.ksize;
    const int ctiles = (d.ldcin + TC - 1) / TC, ntiles = (d.ldcout + TN - 1) / TN;
    int u = blockIdx.x - d.first_block;
    const int ntile = u % ntiles; u /= ntiles;
    const int ctile = u % ctiles;
    const int tap = u / ctiles;
    const int n0 = ntile * TN, c0 = ctile * TC;
    const int tid = threadIdx.x;
    const float *Wt = d.W + (long)tap * d.cin * d.cout;
    const bool vec_ok = (d.cout & 3) == 0 && (((uintptr_t)d.W) & 15) == 0;
    {   // load: TN / 4 lanes x float4 per row
        constexpr int LPR = TN / 4, RPP = 256 / LPR;
        const int col = (tid % LPR) * 4, r0 = tid / LPR;
#pragma unroll
        for (int p = 0; p < TC / RPP; ++p) {
            const int c = c0 + r0 + p * RPP, nn = n0 + col;
            float v[4] = {0.f, 0.f, 0.f, 0.f};
            if (c < d.cin) {
                if (vec_ok && nn + 3 < d.cout) {
                    const f32x4 t = *reinterpret_cast<const f32x4 *>(Wt + (long)c * d.cout + nn);
                    v[0] = t[0]; v[1] = t[1]; v[2] = t[2]; v[3] = t[3];
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (nn + j < d.cout) v[j] = Wt[(long)c * d.cout + nn + j];
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) tile[r0 + p * RPP][col + j] = v[j];
        }
    }
    __syncthreads();
    filter_tile_emit<T>(d, tile, tap, taps, c0, n0, tid);
}

extern "C" int yolo2_filter_prep_blocks(int ksize, int ldcin, int ldcout) {
    if (ksize < 1 || ldcin < 1 || ldcout < 1) return 0;
    return ksize * ksize * cdiv(ldcin, YOLO2_FILTER_PREP_TILE) * cdiv(ldcout, YOLO2_FILTER_PREP_TILE_N);
}
extern "C" int yolo2_filter_prep_batch(const yolo2_filter_desc *descs_device, int n, int total_blocks, int dtype, void *stream) {
    Y2_CHECK_ARG(descs_device && n > 0 && total_blocks > 0);
    Y2_DISPATCH_DTYPE(dtype, filter_prep_batch_kernel<T><<<total_blocks, 256, 0, (hipStream_t)stream>>>(descs_device, n));
    Y2_CHECK_LAUNCH();
    return YOLO2_OK;
}

// ---- Adam + operand layouts in one pass (round 3).  The Adam kernel streams every weight through registers anyway; the operand
// re-layout (filter_prep_batch_kernel: 268 MB re-read of the f32 masters + one more launch per step) rides on it: a workgroup takes one
// 64 x 64 (c, n) tile of one tap of one layer -- the re-layout's own decomposition, which covers every filter element exactly once --
// updates w / m / v in place (16-byte accesses, the same arithmetic as adam_kernel) and emits both bf16 / f32 operand layouts from the
// fresh values staged in LDS.  The parameters that are not convolution filters (gamma, beta, biases: ~22 k floats in 43 ranges) are
// updated by the extra workgroups at the end of the grid.  Results are bit-identical to yolo2_adam followed by yolo2_filter_prep_batch.
struct Y2AdamArgs { float *params; const float *grads; float *m, *v; float alpha, omb1, omb2, eps, gs; };
template <typename T>
__global__ __launch_bounds__(256) void adam_filter_prep_kernel(const yolo2_filter_desc *__restrict__ descs, int n, int conv_blocks,
                                                               const long *__restrict__ small, const Y2AdamArgs a) {
    if ((int)blockIdx.x >= conv_blocks) {      // a non-filter parameter range [small[2i], small[2i] + small[2i+1])
        const long *r = small + 2 * ((int)blockIdx.x - conv_blocks);
        for (long k = threadIdx.x; k < r[1]; k += 256) {
            const long o = r[0] + k;
            adam_one(a.params[o], a.grads[o], a.m[o], a.v[o], a.alpha, a.omb1, a.omb2, a.eps, a.gs);
        }
        return;
    }
    constexpr int TC = YOLO2_FILTER_PREP_TILE, TN = YOLO2_FILTER_PREP_TILE_N;
    __shared__ float tile[TC][TN + 1];
    int li = 0;
    while (li + 1 < n && (int)blockIdx.x >= descs[li + 1].first_block) ++li;
    const yolo2_filter_desc d = descs[li];
    const int taps = d.ksize * d.ksize;
    const int ctiles = (d.ldcin + TC - 1) / TC, ntiles = (d.ldcout + TN - 1) / TN;
    int u = blockIdx.x - d.first_block;
    const int ntile = u % ntiles; u /= ntiles;
    const int ctile = u % ctiles;
    const int tap = u / ctiles;
    const int n0 = ntile * TN, c0 = ctile * TC;
    const int tid = threadIdx.x;
    const long base = (d.W - a.params) + (long)tap * d.cin * d.cout;       // element offset of this tap's [cin][cout] plane in the arenas
    const bool vec_ok = (d.cout & 3) == 0 && ((base & 3) == 0);
    {
        // TN / 4 lanes x float4 per row: a 128-wide tile reads and writes w / m / v / g in 512-byte runs (round 6: with 64 x 64 tiles the four streams
        // moved in 256-byte runs at 5.5-5.7 TB/s where the linear adam_kernel reaches 6.9)
        constexpr int LPR = TN / 4, RPP = 256 / LPR;
        const int col = (tid % LPR) * 4, r0 = tid / LPR;
#pragma unroll
        for (int p = 0; p < TC / RPP; ++p) {
            const int c = c0 + r0 + p * RPP, nn = n0 + col;
            float w4[4] = {0.f, 0.f, 0.f, 0.f};
            if (c < d.cin) {
                const long o = base + (long)c * d.cout + nn;
                if (vec_ok && nn + 3 < d.cout) {
                    f32x4 wv = *reinterpret_cast<const f32x4 *>(a.params + o), mv = *reinterpret_cast<const f32x4 *>(a.m + o), vv = *reinterpret_cast<const f32x4 *>(a.v + o);
                    const f32x4 gv = *reinterpret_cast<const f32x4 *>(a.grads + o);
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        float wj = wv[j], mj = mv[j], vj = vv[j];
                        adam_one(wj, gv[j], mj, vj, a.alpha, a.omb1, a.omb2, a.eps, a.gs);
                        wv[j] = wj; mv[j] = mj; vv[j] = vj; w4[j] = wj;
                    }
                    *reinterpret_cast<f32x4 *>(a.m + o) = mv;
                    *reinterpret_cast<f32x4 *>(a.v + o) = vv;
                    *reinterpret_cast<f32x4 *>(a.params + o) = wv;
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (nn + j < d.cout) {
                            adam_one(a.params[o + j], a.grads[o + j], a.m[o + j], a.v[o + j], a.alpha, a.omb1, a.omb2, a.eps, a.gs);
                            w4[j] = a.params[o + j];
                        }
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) tile[r0 + p * RPP][col + j] = w4[j];
        }
    }
    __syncthreads();
    filter_tile_emit<T>(d, tile, tap, taps, c0, n0, tid);
}
extern "C" int yolo2_adam_filter_prep(const yolo2_filter_desc *descs_device, int n, int total_blocks, const long *small_ranges_device, int n_small,
                                      float *params, const float *grads, float *m, float *v, float alpha, float beta1, float beta2, float eps,
                                      float gscale, int dtype, void *stream) {
    // (n == 0: only the non-filter ranges -- the last launch of a step whose filters were updated layer by layer during backward)
    Y2_CHECK_ARG(n >= 0 && total_blocks >= 0 && (n > 0) == (total_blocks > 0) && (descs_device || n == 0) && n_small >= 0 && total_blocks + n_small > 0 &&
                 (small_ranges_device || n_small == 0) && params && grads && m && v);
    Y2_CHECK_ARG(((((uintptr_t)params) | ((uintptr_t)grads) | ((uintptr_t)m) | ((uintptr_t)v)) & 15) == 0);
    const Y2AdamArgs a{params, grads, m, v, alpha, 1.0f - beta1, 1.0f - beta2, eps, gscale};
    Y2_DISPATCH_DTYPE(dtype, adam_filter_prep_kernel<T><<<total_blocks + n_small, 256, 0, (hipStream_t)stream>>>(descs_device, n, total_blocks, small_ranges_device, a));
    Y2_CHECK_LAUNCH();
    return YOLO2_OK;
}
