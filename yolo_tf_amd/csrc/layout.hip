// Data movement kernels (gfx950), 16-byte vectors along the NHWC channel axis: 2x2 max pool, reorg, channel copies, add, image standardisation, bf16 wire casts.
#include "common.h"

// ------------------------------------------------------------------------------------------
// max pool 2x2 SAME
// ------------------------------------------------------------------------------------------
template <typename T>
__global__ void maxpool_fwd_kernel(const T *__restrict__ A, T *__restrict__ P, int B, int H, int W, int C, int stride) {
    constexpr int N = Vec16<T>::N;
    const int OH = stride == 2 ? H / 2 : H, OW = stride == 2 ? W / 2 : W;
    const int cgs = C / N;
    const long total = (long)B * OH * OW * cgs;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        int cg = (int)(i % cgs);
        long p = i / cgs;
        int ow = (int)(p % OW);
        long q = p / OW;
        int oh = (int)(q % OH);
        int b = (int)(q / OH);
        const int h0 = oh * stride, w0 = ow * stride;
        Vec16<T> m = ld16(A + (((long)b * H + h0) * W + w0) * C + cg * N);
#pragma unroll
        for (int k = 1; k < 4; ++k) {
            int hh = h0 + (k >> 1), ww = w0 + (k & 1);
            if (hh < H && ww < W) {
                Vec16<T> v = ld16(A + (((long)b * H + hh) * W + ww) * C + cg * N);
#pragma unroll
                for (int j = 0; j < N; ++j) m.set(j, fmaxf(m.get(j), v.get(j)));
            }
        }
        st16(P + p * C + cg * N, m);
    }
}

// stride 2: one thread per pooled chunk writes all four input positions (full overwrite of dA)
template <typename T, bool ACC>      // ACC: dA += (a second writer of the tensor's gradient: passthrough fan-out), rounded to T like a separate add
__global__ void maxpool_bwd_s2_kernel(const T *__restrict__ A, const T *__restrict__ dP, T *dA, int B, int H, int W, int C) {
    constexpr int N = Vec16<T>::N;
    const int OH = H / 2, OW = W / 2, cgs = C / N;
    const long total = (long)B * OH * OW * cgs;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        int cg = (int)(i % cgs);
        long p = i / cgs;
        int ow = (int)(p % OW);
        long q = p / OW;
        int oh = (int)(q % OH);
        int b = (int)(q / OH);
        Vec16<T> v[4], o[4];
        const long base = (((long)b * H + oh * 2) * W + ow * 2) * C + cg * N;
        v[0] = ld16(A + base);
        v[1] = ld16(A + base + C);
        v[2] = ld16(A + base + (long)W * C);
        v[3] = ld16(A + base + (long)W * C + C);
        Vec16<T> g = ld16(dP + p * C + cg * N);
        if (ACC) {
            o[0] = ld16(dA + base);
            o[1] = ld16(dA + base + C);
            o[2] = ld16(dA + base + (long)W * C);
            o[3] = ld16(dA + base + (long)W * C + C);
        }
#pragma unroll
        for (int j = 0; j < N; ++j) {
            float m = fmaxf(fmaxf(v[0].get(j), v[1].get(j)), fmaxf(v[2].get(j), v[3].get(j)));
            int arg = v[0].get(j) == m ? 0 : v[1].get(j) == m ? 1 : v[2].get(j) == m ? 2 : 3;  // first max in scan order
#pragma unroll
            for (int k = 0; k < 4; ++k) o[k].set(j, (ACC ? o[k].get(j) : 0.f) + (k == arg ? g.get(j) : 0.f));
        }
        st16(dA + base, o[0]);
        st16(dA + base + C, o[1]);
        st16(dA + base + (long)W * C, o[2]);
        st16(dA + base + (long)W * C + C, o[3]);
    }
}

// stride 1 (tiny model): one thread per INPUT chunk gathers from the <=4 windows containing it
template <typename T>
__global__ void maxpool_bwd_s1_kernel(const T *__restrict__ A, const T *__restrict__ dP, T *__restrict__ dA, int B, int H, int W, int C) {
    constexpr int N = Vec16<T>::N;
    const int cgs = C / N;
    const long total = (long)B * H * W * cgs;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        int cg = (int)(i % cgs);
        long p = i / cgs;
        int w = (int)(p % W);
        long q = p / W;
        int h = (int)(q % H);
        int b = (int)(q / H);
        float acc[N];
#pragma unroll
        for (int j = 0; j < N; ++j) acc[j] = 0.f;
        for (int oh = h - 1; oh <= h; ++oh) {
            if (oh < 0) continue;
            for (int ow = w - 1; ow <= w; ++ow) {
                if (ow < 0) continue;
                // window (oh, ow) covers (oh..oh+1, ow..ow+1); position of (h, w) inside it:
                const int mypos = (h - oh) * 2 + (w - ow);
                Vec16<T> v[4];
                bool ok[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    int hh = oh + (k >> 1), ww = ow + (k & 1);
                    ok[k] = hh < H && ww < W;
                    v[k] = ok[k] ? ld16(A + (((long)b * H + hh) * W + ww) * C + cg * N) : zero16<T>();
                }
                Vec16<T> g = ld16(dP + (((long)b * H + oh) * W + ow) * C + cg * N);
#pragma unroll
                for (int j = 0; j < N; ++j) {
                    float m = -INFINITY;
#pragma unroll
                    for (int k = 0; k < 4; ++k) if (ok[k]) m = fmaxf(m, v[k].get(j));
                    int arg = 3;
#pragma unroll
                    for (int k = 3; k >= 0; --k) if (ok[k] && v[k].get(j) == m) arg = k;
                    if (arg == mypos) acc[j] += g.get(j);
                }
            }
        }
        Vec16<T> o;
#pragma unroll
        for (int j = 0; j < N; ++j) o.set(j, acc[j]);
        st16(dA + p * C + cg * N, o);
    }
}

extern "C" int yolo2_maxpool_fwd(const void *A, void *P, int B, int H, int W, int C, int stride, int dtype, void *stream) {
    Y2_CHECK_ARG(A && P && B > 0 && H > 0 && W > 0 && C > 0);
    Y2_CHECK_ARG(stride == 1 || (stride == 2 && H % 2 == 0 && W % 2 == 0));
    const int vec = dtype == YOLO2_BF16 ? 8 : 4;
    Y2_CHECK_ARG(C % vec == 0);
    long total = (long)B * (stride == 2 ? H / 2 : H) * (stride == 2 ? W / 2 : W) * (C / vec);
    Y2_DISPATCH_DTYPE(dtype, maxpool_fwd_kernel<T><<<ew_grid(total), 256, 0, (hipStream_t)stream>>>((const T *)A, (T *)P, B, H, W, C, stride));
    Y2_CHECK_LAUNCH();
    return YOLO2_OK;
}
extern "C" int yolo2_maxpool_bwd(const void *A, const void *dP, void *dA, int B, int H, int W, int C, int stride, int dtype, void *stream) {
    Y2_CHECK_ARG(A && dP && dA && B > 0 && H > 0 && W > 0 && C > 0);
    Y2_CHECK_ARG(stride == 1 || (stride == 2 && H % 2 == 0 && W % 2 == 0));
    const int vec = dtype == YOLO2_BF16 ? 8 : 4;
    Y2_CHECK_ARG(C % vec == 0);
    hipStream_t st = (hipStream_t)stream;
    if (stride == 2) {
        long total = (long)B * (H / 2) * (W / 2) * (C / vec);
        Y2_DISPATCH_DTYPE(dtype, maxpool_bwd_s2_kernel<T, false><<<ew_grid(total), 256, 0, st>>>((const T *)A, (const T *)dP, (T *)dA, B, H, W, C));
    } else {
        long total = (long)B * H * W * (C / vec);
        Y2_DISPATCH_DTYPE(dtype, maxpool_bwd_s1_kernel<T><<<ew_grid(total), 256, 0, st>>>((const T *)A, (const T *)dP, (T *)dA, B, H, W, C));
    }
    Y2_CHECK_LAUNCH();
    return YOLO2_OK;
}

// dA += the routed gradient (stride 2): yolo2_maxpool_bwd into a temporary + yolo2_add_inplace in one launch, same rounding
extern "C" int yolo2_maxpool_bwd_acc(const void *A, const void *dP, void *dA, int B, int H, int W, int C, int dtype, void *stream) {
    Y2_CHECK_ARG(A && dP && dA && B > 0 && H > 0 && W > 0 && C > 0 && H % 2 == 0 && W % 2 == 0);
    const int vec = dtype == YOLO2_BF16 ? 8 : 4;
    Y2_CHECK_ARG(C % vec == 0);
    long total = (long)B * (H / 2) * (W / 2) * (C / vec);
    Y2_DISPATCH_DTYPE(dtype, maxpool_bwd_s2_kernel<T, true><<<ew_grid(total), 256, 0, (hipStream_t)stream>>>((const T *)A, (const T *)dP, (T *)dA, B, H, W, C));
    Y2_CHECK_LAUNCH();
    return YOLO2_OK;
}

// ------------------------------------------------------------------------------------------
// reorg (space-to-depth, model/yolo2/function.py:22-29) and channel-slice moves
// ------------------------------------------------------------------------------------------
template <typename T, bool BWD>
__global__ void reorg_kernel(const T *__restrict__ src, T *__restrict__ dst, int B, int H, int W, int C, int ld) {
    // forward: src = in [B,H,W,C], dst = out [B,H/2,W/2,ld];  backward: src = dout (stride ld), dst = din
    constexpr int N = Vec16<T>::N;
    const int OH = H / 2, OW = W / 2, cgs = C / N;
    const long total = (long)B * H * W * cgs;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        int cg = (int)(i % cgs);
        long p = i / cgs;  // input pixel index (b, h, w)
        int w = (int)(p % W);
        long q = p / W;
        int h = (int)(q % H);
        int b = (int)(q / H);
        const long in_off = p * C + cg * N;
        const long out_off = (((long)b * OH + (h >> 1)) * OW + (w >> 1)) * ld + ((h & 1) * 2 + (w & 1)) * C + cg * N;
        if (!BWD) st16(dst + out_off, ld16(src + in_off));
        else st16(dst + in_off, ld16(src + out_off));
    }
}
extern "C" int yolo2_reorg(const void *in, void *out, int B, int H, int W, int C, int ldo, int dtype, void *stream) {
    Y2_CHECK_ARG(in && out && B > 0 && H > 0 && W > 0 && C > 0 && H % 2 == 0 && W % 2 == 0 && ldo >= 4 * C);
    const int vec = dtype == YOLO2_BF16 ? 8 : 4;
    Y2_CHECK_ARG(C % vec == 0 && ldo % vec == 0);
    long total = (long)B * H * W * (C / vec);
    Y2_DISPATCH_DTYPE(dtype, reorg_kernel<T, false><<<ew_grid(total), 256, 0, (hipStream_t)stream>>>((const T *)in, (T *)out, B, H, W, C, ldo));
    Y2_CHECK_LAUNCH();
    return YOLO2_OK;
}
extern "C" int yolo2_reorg_bwd(const void *dout, int ldd, void *din, int B, int H, int W, int C, int dtype, void *stream) {
    Y2_CHECK_ARG(dout && din && B > 0 && H > 0 && W > 0 && C > 0 && H % 2 == 0 && W % 2 == 0 && ldd >= 4 * C);
    const int vec = dtype == YOLO2_BF16 ? 8 : 4;
    Y2_CHECK_ARG(C % vec == 0 && ldd % vec == 0);
    long total = (long)B * H * W * (C / vec);
    Y2_DISPATCH_DTYPE(dtype, reorg_kernel<T, true><<<ew_grid(total), 256, 0, (hipStream_t)stream>>>((const T *)dout, (T *)din, B, H, W, C, ldd));
    Y2_CHECK_LAUNCH();
    return YOLO2_OK;
}

template <typename T>
__global__ void copy_channels_kernel(const T *__restrict__ src, int lds, T *__restrict__ dst, int ldd, long M, int C) {
    constexpr int N = Vec16<T>::N;
    const int cgs = C / N;
    const long total = M * cgs;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        int cg = (int)(i % cgs);
        long r = i / cgs;
        st16(dst + r * ldd + cg * N, ld16(src + r * lds + cg * N));
    }
}
extern "C" int yolo2_copy_channels(const void *src, int lds, void *dst, int ldd, long M, int C, int dtype, void *stream) {
    Y2_CHECK_ARG(src && dst && M > 0 && C > 0 && lds >= C && ldd >= C);
    const int vec = dtype == YOLO2_BF16 ? 8 : 4;
    Y2_CHECK_ARG(C % vec == 0 && lds % vec == 0 && ldd % vec == 0);
    Y2_DISPATCH_DTYPE(dtype, copy_channels_kernel<T><<<ew_grid(M * (C / vec)), 256, 0, (hipStream_t)stream>>>((const T *)src, lds, (T *)dst, ldd, M, C));
    Y2_CHECK_LAUNCH();
    return YOLO2_OK;
}

template <typename T>
__global__ void add_inplace_kernel(T *__restrict__ dst, const T *__restrict__ src, long nvec) {
    constexpr int N = Vec16<T>::N;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < nvec; i += (long)gridDim.x * blockDim.x) {
        Vec16<T> a = ld16(dst + i * N), b = ld16(src + i * N), o;
#pragma unroll
        for (int j = 0; j < N; ++j) o.set(j, a.get(j) + b.get(j));
        st16(dst + i * N, o);
    }
}
extern "C" int yolo2_add_inplace(void *dst, const void *src, long n, int dtype, void *stream) {
    Y2_CHECK_ARG(dst && src && n > 0);
    const int vec = dtype == YOLO2_BF16 ? 8 : 4;
    Y2_CHECK_ARG(n % vec == 0);
    Y2_DISPATCH_DTYPE(dtype, add_inplace_kernel<T><<<ew_grid(n / vec), 256, 0, (hipStream_t)stream>>>((T *)dst, (const T *)src, n / vec));
    Y2_CHECK_LAUNCH();
    return YOLO2_OK;
}

// ------------------------------------------------------------------------------------------
// image prep (tf.image.per_image_standardization, train.py:103; utils/preprocess.py:23-25)
// ------------------------------------------------------------------------------------------
// Two launches, no memset, no atomics (round 3; was memset + atomic sums + apply): every workgroup of the first kernel stores its (sum,
// sum of squares) pair -- f64, 16-byte loads, four independent chains -- into ws[b][block][2]; the second kernel's workgroups each work
// on ONE image and fold that image's Y2_IMG_PARTS partial pairs in their prologue (the finalisation rides in the consumer, as for the
// batch-norm statistics).  The partial layout makes the result independent of scheduling: bit-reproducible run to run.
#define Y2_IMG_PARTS 64
__global__ __launch_bounds__(256) void image_sums_kernel(const float *__restrict__ img, double *__restrict__ ws, long n_per_image) {
    const int b = blockIdx.y;
    const float *p = img + (long)b * n_per_image;
    double s[4] = {0.0, 0.0, 0.0, 0.0}, q[4] = {0.0, 0.0, 0.0, 0.0};
    const long stride = (long)gridDim.x * blockDim.x;
    long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if ((((uintptr_t)p) & 15) == 0) {         // 16-byte loads, 4 independent f64 chains per quantity
        const long n4 = n_per_image >> 2;
        const f32x4 *p4 = reinterpret_cast<const f32x4 *>(p);
        for (; i + 3 * stride < n4; i += 4 * stride) {       // four 16-byte loads in flight per lane (one per iteration left the
            f32x4 v[4];                                       // kernel latency-bound at 1 TB/s)
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = p4[i + u * stride];
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const double d = (double)v[u][j];
                    s[j] += d;
                    q[j] += d * d;
                }
        }
        for (; i < n4; i += stride) {
            const f32x4 v = p4[i];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const double d = (double)v[j];
                s[j] += d;
                q[j] += d * d;
            }
        }
        i = (n4 << 2) + blockIdx.x * (long)blockDim.x + threadIdx.x;
    }
    for (; i < n_per_image; i += stride) {
        const double d = (double)p[i];
        s[0] += d;
        q[0] += d * d;
    }
    __shared__ double red[2][4];
    const double st = wave_sum_d((s[0] + s[1]) + (s[2] + s[3]));
    const double qt = wave_sum_d((q[0] + q[1]) + (q[2] + q[3]));
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = st; red[1][threadIdx.x >> 6] = qt; }
    __syncthreads();
    if (threadIdx.x < 2) {
        const double *r = red[threadIdx.x];
        ws[((long)b * gridDim.x + blockIdx.x) * 2 + threadIdx.x] = (r[0] + r[1]) + (r[2] + r[3]);
    }
}
// grid = (blocks per image, B): the image index is blockIdx.y; parts = partial pairs per image left by image_sums_kernel (mode 0)
template <typename T>
__global__ __launch_bounds__(256) void image_apply_kernel(const float *__restrict__ img, T *__restrict__ out, const double *__restrict__ ws, long HW, int mode, int parts) {
    const int b = blockIdx.y;
    float sub = 0.f, den = 1.f;
    if (mode == 0) {
        __shared__ double red[2][4];
        double a = 0.0, c = 0.0;
        for (int k = threadIdx.x; k < parts; k += 256) { a += ws[((long)b * parts + k) * 2]; c += ws[((long)b * parts + k) * 2 + 1]; }
        a = wave_sum_d(a);
        c = wave_sum_d(c);
        if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = a; red[1][threadIdx.x >> 6] = c; }
        __syncthreads();
        const double sum = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]), sq = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
        const double n = (double)HW * 3.0;
        const double mean = sum / n;
        double var = sq / n - mean * mean;
        if (var < 0) var = 0;
        sub = (float)mean;
        den = fmaxf((float)sqrt(var), (float)(1.0 / sqrt(n)));
    } else if (mode == 1) {
        den = 255.0f;
    }
    const float *pi = img + (long)b * HW * 3;
    T *po = out + (long)b * HW * 8;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < HW; i += (long)gridDim.x * blockDim.x) {
        const float *p = pi + i * 3;
        float v0 = p[0], v1 = p[1], v2 = p[2];
        if (mode != 2) { v0 = (v0 - sub) / den; v1 = (v1 - sub) / den; v2 = (v2 - sub) / den; }
        Vec16<T> o[sizeof(T) == 2 ? 1 : 2];
        if constexpr (sizeof(T) == 2) {
            o[0].set(0, v0); o[0].set(1, v1); o[0].set(2, v2);
#pragma unroll
            for (int j = 3; j < 8; ++j) o[0].set(j, 0.f);
            st16(po + i * 8, o[0]);
        } else {
            o[0].set(0, v0); o[0].set(1, v1); o[0].set(2, v2); o[0].set(3, 0.f);
#pragma unroll
            for (int j = 0; j < 4; ++j) o[1].set(j, 0.f);
            st16(po + i * 8, o[0]);
            st16(po + i * 8 + 4, o[1]);
        }
    }
}
extern "C" int yolo2_image_prep(const float *img, void *out, double *ws, int B, int HW, int mode, int dtype, void *stream) {
    Y2_CHECK_ARG(img && out && B > 0 && HW > 0 && mode >= 0 && mode <= 2 && ((uintptr_t)out & 15) == 0);
    hipStream_t st = (hipStream_t)stream;
    int parts = 0;
    if (mode == 0) {
        Y2_CHECK_ARG(ws);
        parts = Y2_IMG_PARTS;
        image_sums_kernel<<<dim3(parts, B), 256, 0, st>>>(img, ws, (long)HW * 3);
    }
    int gx = (int)(((long)HW + 1023) / 1024);        // ~4 pixels per thread
    if (gx > 256) gx = 256;
    if ((long)gx * B > 8192) gx = 8192 / B > 0 ? 8192 / B : 1;
    Y2_DISPATCH_DTYPE(dtype, image_apply_kernel<T><<<dim3(gx, B), 256, 0, st>>>(img, (T *)out, ws, (long)HW, mode, parts));
    Y2_CHECK_LAUNCH();
    return YOLO2_OK;
}
extern "C" size_t yolo2_image_prep_workspace_bytes(int B) { return (size_t)2 * Y2_IMG_PARTS * (size_t)(B > 0 ? B : 0) * sizeof(double); }

// ---- gradient wire format of the data-parallel exchange (parallel.GradReducer, grad_dtype = bf16): the f32 gradient bucket is rounded
// to bf16 into a wire buffer, all-reduced there (half the xGMI bytes: 134 MB instead of 269 MB per step and rank), and widened back into
// the f32 arena the optimizer reads.  16 bytes per lane on the wide side.
__global__ __launch_bounds__(256) void cast_f32_bf16_kernel(const float *__restrict__ src, bf16 *__restrict__ dst, long n) {
    const long nv = n >> 3, stride = (long)gridDim.x * 256;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nv; i += stride) {
        const f32x4 a = reinterpret_cast<const f32x4 *>(src)[2 * i], b = reinterpret_cast<const f32x4 *>(src)[2 * i + 1];
        bf16x8 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) { o[j] = (bf16)a[j]; o[4 + j] = (bf16)b[j]; }
        reinterpret_cast<bf16x8 *>(dst)[i] = o;
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 7)) dst[(nv << 3) + threadIdx.x] = (bf16)src[(nv << 3) + threadIdx.x];
}
__global__ __launch_bounds__(256) void cast_bf16_f32_kernel(const bf16 *__restrict__ src, float *__restrict__ dst, long n) {
    const long nv = n >> 3, stride = (long)gridDim.x * 256;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nv; i += stride) {
        const bf16x8 v = reinterpret_cast<const bf16x8 *>(src)[i];
        f32x4 a, b;
#pragma unroll
        for (int j = 0; j < 4; ++j) { a[j] = (float)v[j]; b[j] = (float)v[4 + j]; }
        reinterpret_cast<f32x4 *>(dst)[2 * i] = a;
        reinterpret_cast<f32x4 *>(dst)[2 * i + 1] = b;
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 7)) dst[(nv << 3) + threadIdx.x] = (float)src[(nv << 3) + threadIdx.x];
}
extern "C" int yolo2_cast_f32_bf16(const float *src, void *dst, long n, void *stream) {
    Y2_CHECK_ARG(src && dst && n >= 0 && ((uintptr_t)src & 15) == 0 && ((uintptr_t)dst & 15) == 0);
    if (n == 0) return YOLO2_OK;
    cast_f32_bf16_kernel<<<ew_grid((n + 7) / 8), 256, 0, (hipStream_t)stream>>>(src, (bf16 *)dst, n);
    Y2_CHECK_LAUNCH();
    return YOLO2_OK;
}
extern "C" int yolo2_cast_bf16_f32(const void *src, float *dst, long n, void *stream) {
    Y2_CHECK_ARG(src && dst && n >= 0 && ((uintptr_t)src & 15) == 0 && ((uintptr_t)dst & 15) == 0);
    if (n == 0) return YOLO2_OK;
    cast_bf16_f32_kernel<<<ew_grid((n + 7) / 8), 256, 0, (hipStream_t)stream>>>((const bf16 *)src, dst, n);
    Y2_CHECK_LAUNCH();
    return YOLO2_OK;
}
