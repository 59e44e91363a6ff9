// Elementwise kernels of the int8 inference path: calibration abs-max, quantisation, and the byte forms of the
// max pool and the passthrough reorg.  Built with -ffp-contract=off: the quantiser is compared bit for bit against tests/quant_ref.py.
//
//   q = clip(rint(x * inv_s), -127, 127) in f32, NaN -> 0           (symmetric int8; inv_s = float32(1) / s from the host)
//
// Pool and reorg move bytes: tensors they connect share one scale, and max commutes with a monotone quantiser.
#include "common.h"
#include <float.h>
#include <algorithm>

typedef __attribute__((ext_vector_type(16))) signed char i8x16;

__device__ __forceinline__ int8_t y2_quant_i8(float x, float inv_s) {
    float q = rintf(x * inv_s);
    q = q != q ? 0.f : fminf(fmaxf(q, -127.f), 127.f);
    return (int8_t)(int)q;
}

// ---- abs-max of a list of tensors: grid (ABSMAX_BLOCKS, njobs) ---------------------------------------------------------------------------
#define ABSMAX_BLOCKS 128
__global__ __launch_bounds__(256) void absmax_kernel(const yolo2_absmax_job *__restrict__ jobs, unsigned *__restrict__ out) {
    const yolo2_absmax_job job = jobs[blockIdx.y];
    const long long total = job.rows * job.c;
    unsigned best = 0u, bad = 0u;
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < total; i += 256ll * ABSMAX_BLOCKS) {
        const long long idx = job.ld == job.c ? i : (i / job.c) * job.ld + i % job.c;
        const float a = fabsf(job.dtype == YOLO2_BF16 ? (float)reinterpret_cast<const bf16 *>(job.base)[idx] : reinterpret_cast<const float *>(job.base)[idx]);
        if (a <= FLT_MAX) best = max(best, __builtin_bit_cast(unsigned, a));      // non-negative floats order like their bit patterns
        else ++bad;                                                                // inf or NaN: ignored and counted
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        best = max(best, (unsigned)__shfl_xor((int)best, o, 64));
        bad += (unsigned)__shfl_xor((int)bad, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        if (best) atomicMax(out + 2 * job.slot, best);
        if (bad) atomicAdd(out + 2 * job.slot + 1, bad);
    }
}

extern "C" int yolo2_absmax(const yolo2_absmax_job *jobs, int njobs, unsigned *out, void *stream) {
    Y2_CHECK_ARG(jobs && out && njobs > 0 && njobs <= 65535);
    absmax_kernel<<<dim3(ABSMAX_BLOCKS, (unsigned)njobs), dim3(256), 0, (hipStream_t)stream>>>(jobs, out);
    Y2_CHECK_LAUNCH();
    return YOLO2_OK;
}

// ---- quantise ------------------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void quantize_kernel(const T *__restrict__ X, int ldx, int8_t *__restrict__ Q, int ldq, long rows, int c, float inv_s) {
    const long total = rows * c;
    for (long i = blockIdx.x * 256l + threadIdx.x; i < total; i += 256l * gridDim.x) {
        const long r = i / c;
        const int j = (int)(i - r * c);
        Q[r * ldq + j] = y2_quant_i8((float)X[r * ldx + j], inv_s);
    }
}

extern "C" int yolo2_quantize(const void *X, int ldx, void *Q, int ldq, long rows, int c, float inv_s, int dtype, void *stream) {
    Y2_CHECK_ARG(X && Q && rows > 0 && c > 0 && ldx >= c && ldq >= c);
    Y2_CHECK_ARG(rows <= (1L << 40) / c);
    const unsigned grid = (unsigned)std::min<long>((rows * c + 255) / 256, 1L << 16);
    Y2_DISPATCH_DTYPE(dtype, quantize_kernel<T><<<dim3(grid), dim3(256), 0, (hipStream_t)stream>>>((const T *)X, ldx, (int8_t *)Q, ldq, rows, c, inv_s));
    Y2_CHECK_LAUNCH();
    return YOLO2_OK;
}

// ---- 2x2 SAME max pool on bytes, stride 2 or 1 (the window is clipped at the bottom / right edge) -----------------------------------------
// V = bytes per thread: 16 when the channel count and both strides are multiples of 16 and the pointers are aligned, else 1
template <int V>
__global__ __launch_bounds__(256) void maxpool_i8_kernel(const int8_t *__restrict__ A, int lda, int8_t *__restrict__ Pq, int ldp, int B, int H, int W, int C,
                                                         int stride, int OH, int OW) {
    const int cv = C / V;
    const long total = (long)B * OH * OW * cv;
    for (long i = blockIdx.x * 256l + threadIdx.x; i < total; i += 256l * gridDim.x) {
        const long pix = i / cv;
        const int c = (int)(i - pix * cv) * V;
        const int ox = (int)(pix % OW);
        const long t = pix / OW;
        const int oy = (int)(t % OH);
        const long b = t / OH;
        const int y0 = oy * stride, x0 = ox * stride;
        const int y1 = min(y0 + 1, H - 1), x1 = min(x0 + 1, W - 1);
        const int8_t *base = A + b * H * W * (long)lda + c;
        const long o = pix * ldp + c;
        if (V == 16) {
            const i8x16 a = *reinterpret_cast<const i8x16 *>(base + ((long)y0 * W + x0) * lda), b_ = *reinterpret_cast<const i8x16 *>(base + ((long)y0 * W + x1) * lda);
            const i8x16 c_ = *reinterpret_cast<const i8x16 *>(base + ((long)y1 * W + x0) * lda), d = *reinterpret_cast<const i8x16 *>(base + ((long)y1 * W + x1) * lda);
            *reinterpret_cast<i8x16 *>(Pq + o) = __builtin_elementwise_max(__builtin_elementwise_max(a, b_), __builtin_elementwise_max(c_, d));
        } else {
            const int8_t a = base[((long)y0 * W + x0) * lda], b_ = base[((long)y0 * W + x1) * lda];
            const int8_t c_ = base[((long)y1 * W + x0) * lda], d = base[((long)y1 * W + x1) * lda];
            Pq[o] = max(max(a, b_), max(c_, d));
        }
    }
}

extern "C" int yolo2_maxpool_i8(const void *A, int lda, void *Pq, int ldp, int B, int H, int W, int C, int stride, void *stream) {
    Y2_CHECK_ARG(A && Pq && B > 0 && H > 0 && W > 0 && C > 0 && lda >= C && ldp >= C);
    Y2_CHECK_ARG(stride == 1 || stride == 2);
    const int OH = stride == 2 ? (H + 1) / 2 : H, OW = stride == 2 ? (W + 1) / 2 : W;
    const bool vec = C % 16 == 0 && lda % 16 == 0 && ldp % 16 == 0 && (((uintptr_t)A | (uintptr_t)Pq) & 15) == 0;
    const long total = (long)B * OH * OW * (vec ? C / 16 : C);
    const unsigned grid = (unsigned)std::min<long>((total + 255) / 256, 1L << 16);
    if (vec) maxpool_i8_kernel<16><<<dim3(grid), dim3(256), 0, (hipStream_t)stream>>>((const int8_t *)A, lda, (int8_t *)Pq, ldp, B, H, W, C, stride, OH, OW);
    else maxpool_i8_kernel<1><<<dim3(grid), dim3(256), 0, (hipStream_t)stream>>>((const int8_t *)A, lda, (int8_t *)Pq, ldp, B, H, W, C, stride, OH, OW);
    Y2_CHECK_LAUNCH();
    return YOLO2_OK;
}

// ---- reorg on bytes: out[b, y, x, (sy*2 + sx)*C + c] = in[b, 2y + sy, 2x + sx, c]; `in` dense, `out` with pixel stride ldo -------------------
template <int V>
__global__ __launch_bounds__(256) void reorg_i8_kernel(const int8_t *__restrict__ in, int8_t *__restrict__ out, int B, int H, int W, int C, int ldo) {
    const int cv = C / V;
    const long total = (long)B * H * W * cv;
    for (long i = blockIdx.x * 256l + threadIdx.x; i < total; i += 256l * gridDim.x) {
        const long pix = i / cv;
        const int c = (int)(i - pix * cv) * V;
        const int x = (int)(pix % W);
        const long t = pix / W;
        const int y = (int)(t % H);
        const long b = t / H;
        const long o = ((b * (H / 2) + y / 2) * (W / 2) + x / 2) * ldo + ((y & 1) * 2 + (x & 1)) * C + c;
        if (V == 16) *reinterpret_cast<i8x16 *>(out + o) = *reinterpret_cast<const i8x16 *>(in + pix * C + c);
        else out[o] = in[pix * C + c];
    }
}

extern "C" int yolo2_reorg_i8(const void *in, void *out, int B, int H, int W, int C, int ldo, void *stream) {
    Y2_CHECK_ARG(in && out && B > 0 && H > 0 && W > 0 && C > 0);
    Y2_CHECK_ARG(H % 2 == 0 && W % 2 == 0 && ldo >= 4 * C);
    const bool vec = C % 16 == 0 && ldo % 16 == 0 && (((uintptr_t)in | (uintptr_t)out) & 15) == 0;
    const long total = (long)B * H * W * (vec ? C / 16 : C);
    const unsigned grid = (unsigned)std::min<long>((total + 255) / 256, 1L << 16);
    if (vec) reorg_i8_kernel<16><<<dim3(grid), dim3(256), 0, (hipStream_t)stream>>>((const int8_t *)in, (int8_t *)out, B, H, W, C, ldo);
    else reorg_i8_kernel<1><<<dim3(grid), dim3(256), 0, (hipStream_t)stream>>>((const int8_t *)in, (int8_t *)out, B, H, W, C, ldo);
    Y2_CHECK_LAUNCH();
    return YOLO2_OK;
}
