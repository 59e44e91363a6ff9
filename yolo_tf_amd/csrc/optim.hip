// Optimizers, gradient clipping and the small arena kernels (scale, zero ranges, BN folding), gfx950.  Adam fused with the filter re-layout: filter_prep.hip.
#include "common.h"
#include "adam.h"

// ------------------------------------------------------------------------------------------
// optimizers, TF-1.0 Apply* semantics (train.py:70-80); g is scaled by gscale first (1/world
// for data-parallel gradient averaging)
// ------------------------------------------------------------------------------------------
#define OPT_LOOP(n) for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < (n); i += (long)gridDim.x * blockDim.x)
// the dominant optimizer: 28 B of HBM traffic per parameter.  16-byte accesses when the four arenas are 16-byte aligned
// (they are: the engine's arenas and every all-reduce bucket start on a multiple of 4 elements), scalar tail otherwise.
__global__ __launch_bounds__(256) void adam_kernel(float *w, const float *g, float *m, float *v, long n, float alpha, float omb1, float omb2, float eps, float gs) {
    const long stride = (long)gridDim.x * blockDim.x;
    long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
    long done = 0;
    if (((((uintptr_t)w) | ((uintptr_t)g) | ((uintptr_t)m) | ((uintptr_t)v)) & 15) == 0) {
        const long n4 = n >> 2;
        f32x4 *w4 = reinterpret_cast<f32x4 *>(w), *m4 = reinterpret_cast<f32x4 *>(m), *v4 = reinterpret_cast<f32x4 *>(v);
        const f32x4 *g4 = reinterpret_cast<const f32x4 *>(g);
        for (long k = i; k < n4; k += stride) {
            f32x4 wv = w4[k], mv = m4[k], vv = v4[k];
            const f32x4 gv = g4[k];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float wj = wv[j], mj = mv[j], vj = vv[j];
                adam_one(wj, gv[j], mj, vj, alpha, omb1, omb2, eps, gs);
                wv[j] = wj; mv[j] = mj; vv[j] = vj;
            }
            m4[k] = mv;
            v4[k] = vv;
            w4[k] = wv;
        }
        done = n4 << 2;
    }
    for (long k = done + i; k < n; k += stride) adam_one(w[k], g[k], m[k], v[k], alpha, omb1, omb2, eps, gs);
}
__global__ void momentum_kernel(float *w, const float *g, float *acc, long n, float lr, float mom, float gs) {
    OPT_LOOP(n) {
        float a = acc[i] * mom + g[i] * gs;
        acc[i] = a;
        w[i] = w[i] - lr * a;
    }
}
__global__ void sgd_kernel(float *w, const float *g, long n, float lr, float gs) {
    OPT_LOOP(n) w[i] = w[i] - lr * (g[i] * gs);
}
__global__ void rmsprop_kernel(float *w, const float *g, float *ms, float *mom, long n, float lr, float omd, float momentum, float eps, float gs) {
    OPT_LOOP(n) {
        float gi = g[i] * gs;
        float s = ms[i] + (gi * gi - ms[i]) * omd;
        float mo = mom[i] * momentum + lr * gi / sqrtf(s + eps);
        ms[i] = s;
        mom[i] = mo;
        w[i] = w[i] - mo;
    }
}
__global__ void adagrad_kernel(float *w, const float *g, float *acc, long n, float lr, float gs) {
    OPT_LOOP(n) {
        float gi = g[i] * gs;
        float a = acc[i] + gi * gi;
        acc[i] = a;
        w[i] = w[i] - lr * gi / sqrtf(a);
    }
}
__global__ void adadelta_kernel(float *w, const float *g, float *acc, float *accu, long n, float lr, float rho, float eps, float gs) {
    OPT_LOOP(n) {
        float gi = g[i] * gs;
        float a = acc[i] * rho + gi * gi * (1.0f - rho);
        float u = sqrtf(accu[i] + eps) / sqrtf(a + eps) * gi;
        accu[i] = accu[i] * rho + u * u * (1.0f - rho);
        acc[i] = a;
        w[i] = w[i] - lr * u;
    }
}
// [TF-sem] ApplyFtrl (tf.train.FtrlOptimizer, reference train.py:78): accum starts at initial_accumulator_value, linear at 0.
//   new_accum = accum + g^2;  linear += g - (new_accum^-p - accum^-p) / lr * w;   (p = learning_rate_power, sqrt when p = -0.5)
//   w = |linear| > l1 ? (l1 * sign(linear) - linear) / (new_accum^-p / lr + 2 * l2) : 0
__global__ void ftrl_kernel(float *w, const float *g, float *accum, float *linear, long n, float lr, float lr_power, float l1, float l2, float gs) {
    const bool half = lr_power == -0.5f;
    OPT_LOOP(n) {
        const float gi = g[i] * gs;
        const float a = accum[i], na = a + gi * gi;
        const float pa = half ? sqrtf(a) : powf(a, -lr_power), pna = half ? sqrtf(na) : powf(na, -lr_power);
        const float li = linear[i] + (gi - (pna - pa) / lr * w[i]);
        const float sgn = li > 0.f ? 1.f : (li < 0.f ? -1.f : 0.f);
        const float x = l1 * sgn - li;
        const float y = pna / lr + 2.0f * l2;
        w[i] = fabsf(li) > l1 ? x / y : 0.f;
        linear[i] = li;
        accum[i] = na;
    }
}
__global__ void scale_kernel(float *x, long n, float sc) {
    OPT_LOOP(n) x[i] = x[i] * sc;
}
// inference-time batch-norm folding: Wf[r, n] = W[r, n] * s[n], bias[n] = beta[n] - mean[n] * s[n], s = gamma / sqrt(var + eps)
__global__ void bn_fold_kernel(const float *__restrict__ W, const float *__restrict__ gamma, const float *__restrict__ beta, const float *__restrict__ mean,
                               const float *__restrict__ var, float *__restrict__ Wf, float *__restrict__ bias, long rows, int C, float eps) {
    const long total = rows * C;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int n = (int)(i % C);
        const float sc = gamma[n] / sqrtf(var[n] + eps);
        Wf[i] = W[i] * sc;
        if (i < C) bias[n] = beta[n] - mean[n] * sc;
    }
}

extern "C" int yolo2_ftrl(float *w, const float *g, float *accum, float *linear, long n, float lr, float lr_power, float l1, float l2, float gscale, void *stream) {
    Y2_CHECK_ARG(w && g && accum && linear && n > 0 && lr > 0.f && lr_power <= 0.f);
    ftrl_kernel<<<ew_grid(n / 4 + 1), 256, 0, (hipStream_t)stream>>>(w, g, accum, linear, n, lr, lr_power, l1, l2, gscale);
    Y2_CHECK_LAUNCH();
    return YOLO2_OK;
}
extern "C" int yolo2_scale(float *x, long n, float scale, void *stream) {
    Y2_CHECK_ARG(x && n > 0);
    scale_kernel<<<ew_grid(n / 4 + 1), 256, 0, (hipStream_t)stream>>>(x, n, scale);
    Y2_CHECK_LAUNCH();
    return YOLO2_OK;
}
// up to Y2_ZR_MAX ranges per launch, passed by value (one launch instead of one hipMemsetAsync node per range: 5 launches per training step)
#define Y2_ZR_MAX 16
struct Y2ZeroRanges { long a[Y2_ZR_MAX], b[Y2_ZR_MAX]; int n; };
__global__ __launch_bounds__(256) void zero_ranges_kernel(float *__restrict__ x, const Y2ZeroRanges zr) {
    const long tid = blockIdx.x * (long)blockDim.x + threadIdx.x, stride = (long)gridDim.x * blockDim.x;
    for (int r = 0; r < zr.n; ++r) {
        const long a = zr.a[r], b = zr.b[r];
        const long a4 = (a + 3) & ~3L, b4 = b & ~3L;            // 16-byte body, scalar edges
        if (a4 <= b4) {
            const f32x4 z = {0.f, 0.f, 0.f, 0.f};
            for (long i = a4 / 4 + tid; i < b4 / 4; i += stride) reinterpret_cast<f32x4 *>(x)[i] = z;
            for (long i = a + tid; i < a4; i += stride) x[i] = 0.f;
            for (long i = b4 + tid; i < b; i += stride) x[i] = 0.f;
        } else {
            for (long i = a + tid; i < b; i += stride) x[i] = 0.f;
        }
    }
}
extern "C" int yolo2_zero_ranges(float *x, const long *ranges_host, int nranges, void *stream) {
    Y2_CHECK_ARG(x && (nranges == 0 || ranges_host) && nranges >= 0 && ((uintptr_t)x & 15) == 0);
    for (int i0 = 0; i0 < nranges; i0 += Y2_ZR_MAX) {
        Y2ZeroRanges zr;
        zr.n = 0;
        long total = 0;
        for (int i = i0; i < nranges && i < i0 + Y2_ZR_MAX; ++i) {
            const long a = ranges_host[2 * i], b = ranges_host[2 * i + 1];
            Y2_CHECK_ARG(a >= 0 && b >= a);
            if (b > a) { zr.a[zr.n] = a; zr.b[zr.n] = b; ++zr.n; total += b - a; }
        }
        if (zr.n) zero_ranges_kernel<<<ew_grid(total / 4 + 1), 256, 0, (hipStream_t)stream>>>(x, zr);
    }
    Y2_CHECK_LAUNCH();
    return YOLO2_OK;
}
extern "C" int yolo2_bn_fold(const float *W, const float *gamma, const float *beta, const float *moving_mean, const float *moving_var, float *Wf,
                             float *bias, long rows, int C, float eps, void *stream) {
    Y2_CHECK_ARG(W && gamma && beta && moving_mean && moving_var && Wf && bias && rows > 0 && C > 0);
    bn_fold_kernel<<<ew_grid(rows * C), 256, 0, (hipStream_t)stream>>>(W, gamma, beta, moving_mean, moving_var, Wf, bias, rows, C, eps);
    Y2_CHECK_LAUNCH();
    return YOLO2_OK;
}

extern "C" int yolo2_adam(float *w, const float *g, float *m, float *v, long n, float alpha, float beta1, float beta2, float eps, float gscale, void *stream) {
    Y2_CHECK_ARG(w && g && m && v && n > 0);
    adam_kernel<<<ew_grid(n / 4 + 1), 256, 0, (hipStream_t)stream>>>(w, g, m, v, n, alpha, 1.0f - beta1, 1.0f - beta2, eps, gscale);
    Y2_CHECK_LAUNCH();
    return YOLO2_OK;
}
extern "C" int yolo2_momentum(float *w, const float *g, float *acc, long n, float lr, float momentum, float gscale, void *stream) {
    Y2_CHECK_ARG(w && g && acc && n > 0);
    momentum_kernel<<<ew_grid(n / 4 + 1), 256, 0, (hipStream_t)stream>>>(w, g, acc, n, lr, momentum, gscale);
    Y2_CHECK_LAUNCH();
    return YOLO2_OK;
}
extern "C" int yolo2_sgd(float *w, const float *g, long n, float lr, float gscale, void *stream) {
    Y2_CHECK_ARG(w && g && n > 0);
    sgd_kernel<<<ew_grid(n / 4 + 1), 256, 0, (hipStream_t)stream>>>(w, g, n, lr, gscale);
    Y2_CHECK_LAUNCH();
    return YOLO2_OK;
}
extern "C" int yolo2_rmsprop(float *w, const float *g, float *ms, float *mom, long n, float lr, float decay, float momentum, float eps, float gscale, void *stream) {
    Y2_CHECK_ARG(w && g && ms && mom && n > 0);
    rmsprop_kernel<<<ew_grid(n / 4 + 1), 256, 0, (hipStream_t)stream>>>(w, g, ms, mom, n, lr, 1.0f - decay, momentum, eps, gscale);
    Y2_CHECK_LAUNCH();
    return YOLO2_OK;
}
extern "C" int yolo2_adagrad(float *w, const float *g, float *acc, long n, float lr, float gscale, void *stream) {
    Y2_CHECK_ARG(w && g && acc && n > 0);
    adagrad_kernel<<<ew_grid(n / 4 + 1), 256, 0, (hipStream_t)stream>>>(w, g, acc, n, lr, gscale);
    Y2_CHECK_LAUNCH();
    return YOLO2_OK;
}
extern "C" int yolo2_adadelta(float *w, const float *g, float *acc, float *acc_update, long n, float lr, float rho, float eps, float gscale, void *stream) {
    Y2_CHECK_ARG(w && g && acc && acc_update && n > 0);
    adadelta_kernel<<<ew_grid(n / 4 + 1), 256, 0, (hipStream_t)stream>>>(w, g, acc, acc_update, n, lr, rho, eps, gscale);
    Y2_CHECK_LAUNCH();
    return YOLO2_OK;
}

// per-tensor clip_by_norm: one block row per segment (grid.y = segment), two passes
// [TF-sem] tf.clip_by_norm: g * clip / max(norm, clip).  fmaxf returns clip for a NaN norm, which would leave a tensor that holds a NaN unscaled;
// TF's maximum (and the oracle's) keeps the NaN and the whole tensor becomes NaN.  One select per workgroup, nothing per element.
__device__ __forceinline__ float clip_scale(float norm, float clip) { return norm == norm ? clip / fmaxf(norm, clip) : norm; }
__global__ void seg_sumsq_kernel(const float *__restrict__ g, const long *__restrict__ seg_off, double *__restrict__ ws) {
    const int s = blockIdx.y;
    const long beg = seg_off[s], end = seg_off[s + 1];
    double acc = 0.0;
    for (long i = beg + blockIdx.x * (long)blockDim.x + threadIdx.x; i < end; i += (long)gridDim.x * blockDim.x) {
        double v = (double)g[i];
        acc += v * v;
    }
    acc = wave_sum_d(acc);
    if ((threadIdx.x & 63) == 0 && acc != 0.0) atomicAdd(ws + s, acc);
}
// fixed-order, two-level form (deterministic mode, yolo2_clip_by_norm_fixed): the same 64 workgroups per segment as above, but workgroup b STORES its sum
// into part[s][b] -- thread chains over a fixed stride, wave_sum_d's fixed butterfly, the four wave sums added in wave order -- and the scale pass adds a
// segment's 64 partials in index order (every thread the same 64 loads from L2).  One writer per partial, no atomic, no clearing.
#define Y2_CLIP_PARTS 64
__global__ __launch_bounds__(256) void seg_sumsq_part_kernel(const float *__restrict__ g, const long *__restrict__ seg_off, double *__restrict__ part) {
    __shared__ double wsum[4];
    const int s = blockIdx.y;
    const long beg = seg_off[s], end = seg_off[s + 1];
    double acc = 0.0;
    for (long i = beg + blockIdx.x * 256L + threadIdx.x; i < end; i += (long)Y2_CLIP_PARTS * 256) {
        const double v = (double)g[i];
        acc += v * v;
    }
    acc = wave_sum_d(acc);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) part[(long)s * Y2_CLIP_PARTS + blockIdx.x] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}
__global__ void seg_scale_fixed_kernel(float *__restrict__ g, const long *__restrict__ seg_off, const double *__restrict__ part, float clip) {
    const int s = blockIdx.y;
    const long beg = seg_off[s], end = seg_off[s + 1];
    double t = 0.0;
    for (int b = 0; b < Y2_CLIP_PARTS; ++b) t += part[(long)s * Y2_CLIP_PARTS + b];
    const float norm = (float)sqrt(t);
    const float scale = clip_scale(norm, clip);
    if (scale == 1.0f) return;
    for (long i = beg + blockIdx.x * (long)blockDim.x + threadIdx.x; i < end; i += (long)gridDim.x * blockDim.x) g[i] = g[i] * scale;
}
__global__ void seg_scale_kernel(float *__restrict__ g, const long *__restrict__ seg_off, const double *__restrict__ ws, float clip) {
    const int s = blockIdx.y;
    const long beg = seg_off[s], end = seg_off[s + 1];
    const float norm = (float)sqrt(ws[s]);
    const float scale = clip_scale(norm, clip);
    if (scale == 1.0f) return;
    for (long i = beg + blockIdx.x * (long)blockDim.x + threadIdx.x; i < end; i += (long)gridDim.x * blockDim.x) g[i] = g[i] * scale;
}
extern "C" int yolo2_clip_by_norm(float *g, const long *seg_off, int nseg, float clip, double *ws, void *stream) {
    Y2_CHECK_ARG(g && seg_off && ws && nseg > 0 && clip > 0.f);
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(ws, 0, sizeof(double) * nseg, st) != hipSuccess) { yolo2_set_error("clip_by_norm: memset failed"); return YOLO2_E_LAUNCH; }
    dim3 grid(64, nseg);
    seg_sumsq_kernel<<<grid, 256, 0, st>>>(g, seg_off, ws);
    seg_scale_kernel<<<grid, 256, 0, st>>>(g, seg_off, ws, clip);
    Y2_CHECK_LAUNCH();
    return YOLO2_OK;
}

extern "C" size_t yolo2_clip_workspace_bytes(int nseg) { return (size_t)(nseg > 0 ? nseg : 0) * sizeof(double); }
extern "C" size_t yolo2_clip_fixed_workspace_bytes(int nseg) { return (size_t)(nseg > 0 ? nseg : 0) * Y2_CLIP_PARTS * sizeof(double); }
extern "C" int yolo2_clip_by_norm_fixed(float *g, const long *seg_off, int nseg, float clip, double *ws, size_t ws_bytes, void *stream) {
    Y2_CHECK_ARG(g && seg_off && ws && nseg > 0 && clip > 0.f && ws_bytes >= yolo2_clip_fixed_workspace_bytes(nseg));
    hipStream_t st = (hipStream_t)stream;
    dim3 grid(Y2_CLIP_PARTS, nseg);
    seg_sumsq_part_kernel<<<grid, 256, 0, st>>>(g, seg_off, ws);
    seg_scale_fixed_kernel<<<grid, 256, 0, st>>>(g, seg_off, ws, clip);
    Y2_CHECK_LAUNCH();
    return YOLO2_OK;
}
