// BN apply + leaky ReLU (+ 2x2 max pool), forward and backward (gfx950), HBM-bound: 16-byte vectors with lanes along the NHWC channel axis, per-channel
// constants in registers.  Two-launch forms (statistics: bn_stats.hip) and the consumers that finish the partial rows in their prologue (*_fin).
#include "common.h"
#include "bn_leaky.h"
#include "colsum.h"

template <typename T>
__global__ __launch_bounds__(256) void bn_leaky_kernel(const T *__restrict__ Y, const float *__restrict__ mean, const float *__restrict__ var,
                                                       const float *__restrict__ gamma, const float *__restrict__ beta, T *__restrict__ A,
                                                       long M, int C, int lda, float eps, float alpha) {
    constexpr int N = Vec16<T>::N;
    RowMap rm(C, N);
    if (!rm.active) return;
    float mu[N], sc[N], bt[N];
#pragma unroll
    for (int j = 0; j < N; ++j) {
        int c = rm.cg * N + j;
        mu[j] = mean[c];
        sc[j] = bn_inv_std(var[c], eps) * gamma[c];
        bt[j] = beta[c];
    }
    for (long r = (long)blockIdx.x * rm.rpp + rm.rs; r < M; r += (long)gridDim.x * rm.rpp) {
        Vec16<T> v = ld16(Y + r * C + rm.cg * N), o;
#pragma unroll
        for (int j = 0; j < N; ++j) o.set(j, bn_leaky(v.get(j), mu[j], sc[j], bt[j], alpha));
        st16(A + r * lda + rm.cg * N, o);
    }
}

static int rowmap_grid(long M, int C, int vec, int rows_per_thread) {
    int tpr = C / vec, rpp = 256 / tpr;
    if (rpp < 1) rpp = 1;
    long g = (M + (long)rpp * rows_per_thread - 1) / ((long)rpp * rows_per_thread);
    if (g > 4096) g = 4096;
    if (g < 1) g = 1;
    return (int)g;
}

extern "C" int yolo2_bn_leaky(const void *Y, const float *mean, const float *var, const float *gamma, const float *beta,
                              void *A, long M, int C, int lda, float eps, float alpha, int dtype, void *stream) {
    Y2_CHECK_ARG(Y && mean && var && gamma && beta && A && M > 0 && C > 0 && lda >= C);
    const int vec = dtype == YOLO2_BF16 ? 8 : 4;
    Y2_CHECK_ARG(C % vec == 0 && C / vec <= 256 && lda % vec == 0);
    int grid = rowmap_grid(M, C, vec, 4);
    Y2_DISPATCH_DTYPE(dtype, bn_leaky_kernel<T><<<grid, 256, 0, (hipStream_t)stream>>>((const T *)Y, mean, var, gamma, beta, (T *)A, M, C, lda, eps, alpha));
    Y2_CHECK_LAUNCH();
    return YOLO2_OK;
}

template <typename T>
__global__ __launch_bounds__(256) void bn_bwd_reduce_kernel(const T *__restrict__ dA, int ldda, const T *__restrict__ Y, const float *__restrict__ mean,
                                                            const float *__restrict__ var, const float *__restrict__ gamma, const float *__restrict__ beta,
                                                            float *__restrict__ ws, long M, int C, float eps, float alpha) {
    constexpr int N = Vec16<T>::N;
    RowMap rm(C, N);
    float part[2][N];
    float mu[N], inv[N], ga[N], bt[N];
#pragma unroll
    for (int j = 0; j < N; ++j) {
        part[0][j] = part[1][j] = 0.f;
        int c = rm.cg * N + j;
        bool ok = rm.active;
        mu[j] = ok ? mean[c] : 0.f;
        inv[j] = ok ? bn_inv_std(var[c], eps) : 0.f;
        ga[j] = ok ? gamma[c] : 0.f;
        bt[j] = ok ? beta[c] : 0.f;
    }
    if (rm.active) {
        const long step = (long)gridDim.x * rm.rpp;
        long r = (long)blockIdx.x * rm.rpp + rm.rs;
        auto accum = [&](const Vec16<T> &y, const Vec16<T> &d) {
#pragma unroll
            for (int j = 0; j < N; ++j) {
                const BnBwdTerm t = bn_leaky_bwd(y.get(j), d.get(j), mu[j], inv[j], ga[j], bt[j], alpha);
                part[0][j] += t.g * t.xh;  // dgamma
                part[1][j] += t.g;         // dbeta
            }
        };
        for (; r + 3 * step < M; r += 4 * step) {          // 8 independent 16-byte loads in flight per lane
            Vec16<T> y[4], d[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                y[u] = ld16(Y + (r + u * step) * C + rm.cg * N);
                d[u] = ld16(dA + (r + u * step) * ldda + rm.cg * N);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) accum(y[u], d[u]);
        }
        for (; r < M; r += step) {
            Vec16<T> y = ld16(Y + r * C + rm.cg * N), d = ld16(dA + r * ldda + rm.cg * N);
            accum(y, d);
        }
    }
    block_colsum_store<N, 2>(part, rm, C, ws, gridDim.x);
}
extern "C" int yolo2_bn_leaky_bwd_reduce(const void *dA, int ldda, const void *Y, const float *mean, const float *var, const float *gamma,
                                         const float *beta, float *dgamma, float *dbeta, double *ws, long M, int C, float eps, float alpha,
                                         int dtype, void *stream) {
    Y2_CHECK_ARG(dA && Y && mean && var && gamma && beta && dgamma && dbeta && ws && M > 0 && C > 0 && ldda >= C);
    const int vec = dtype == YOLO2_BF16 ? 8 : 4;
    Y2_CHECK_ARG(C % vec == 0 && C / vec <= 256 && ldda % vec == 0);
    hipStream_t st = (hipStream_t)stream;
    const int nb = colsum_grid(M, C, vec);
    float *part = (float *)ws;
    Y2_DISPATCH_DTYPE(dtype, bn_bwd_reduce_kernel<T><<<nb, 256, 0, st>>>((const T *)dA, ldda, (const T *)Y, mean, var, gamma, beta, part, M, C, eps, alpha));
    reduce_finalize_kernel<1><<<cdiv(C, 16), 256, 0, st>>>(part, nb, C, M, dgamma, dbeta, C);
    Y2_CHECK_LAUNCH();
    return YOLO2_OK;
}

template <typename T>
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const T *__restrict__ dA, int ldda, const T *__restrict__ Y, const float *__restrict__ mean,
                                                           const float *__restrict__ var, const float *__restrict__ gamma, const float *__restrict__ beta,
                                                           const float *__restrict__ dgamma, const float *__restrict__ dbeta, T *__restrict__ dY,
                                                           long M, int C, float eps, float alpha) {
    constexpr int N = Vec16<T>::N;
    RowMap rm(C, N);
    if (!rm.active) return;
    const float invM = 1.0f / (float)M;
    float mu[N], inv[N], ga[N], bt[N], dgm[N], dbm[N];
#pragma unroll
    for (int j = 0; j < N; ++j) {
        int c = rm.cg * N + j;
        mu[j] = mean[c];
        inv[j] = bn_inv_std(var[c], eps);
        ga[j] = gamma[c];
        bt[j] = beta[c];
        dgm[j] = dgamma[c] * invM;
        dbm[j] = dbeta[c] * invM;
    }
    for (long r = (long)blockIdx.x * rm.rpp + rm.rs; r < M; r += (long)gridDim.x * rm.rpp) {
        Vec16<T> y = ld16(Y + r * C + rm.cg * N), d = ld16(dA + r * ldda + rm.cg * N), o;
#pragma unroll
        for (int j = 0; j < N; ++j) {      // bn_leaky.h bn_leaky_bwd + bn_bwd_apply, spelled out (the helpers change the bf16 form's schedule)
            float xh = (y.get(j) - mu[j]) * inv[j];
            float z = (y.get(j) - mu[j]) * (inv[j] * ga[j]) + bt[j];
            float g = z >= 0.f ? d.get(j) : alpha * d.get(j);
            o.set(j, (ga[j] * inv[j]) * (g - dbm[j] - xh * dgm[j]));
        }
        st16(dY + r * C + rm.cg * N, o);
    }
}

extern "C" int yolo2_bn_leaky_bwd_apply(const void *dA, int ldda, const void *Y, const float *mean, const float *var, const float *gamma,
                                        const float *beta, const float *dgamma, const float *dbeta, void *dY, long M, int C, float eps,
                                        float alpha, int dtype, void *stream) {
    Y2_CHECK_ARG(dA && Y && mean && var && gamma && beta && dgamma && dbeta && dY && M > 0 && C > 0 && ldda >= C);
    const int vec = dtype == YOLO2_BF16 ? 8 : 4;
    Y2_CHECK_ARG(C % vec == 0 && C / vec <= 256 && ldda % vec == 0);
    int grid = rowmap_grid(M, C, vec, 4);
    Y2_DISPATCH_DTYPE(dtype, bn_bwd_apply_kernel<T><<<grid, 256, 0, (hipStream_t)stream>>>((const T *)dA, ldda, (const T *)Y, mean, var, gamma, beta, dgamma, dbeta, (T *)dY, M, C, eps, alpha));
    Y2_CHECK_LAUNCH();
    return YOLO2_OK;
}

// ------------------------------------------------------------------------------------------
// BN + leaky + 2x2/2 max pool in one pass, and its backward (layers whose only consumer is the pool: the
// full-resolution activation and its gradient are never materialised).
//   forward : P = maxpool(leaky(bn(Y))) on the values ROUNDED to T (= what the unfused pair stores and pools),
//             idx = position 0..3 (scan order: (0,0),(0,1),(1,0),(1,1)) of the first maximum, one byte per element
//   backward: dA = dP routed to idx (tf.nn.max_pool gradient, first-max as yolo2_maxpool_bwd), then the BN + leaky
//             backward of yolo2_bn_leaky_bwd_reduce/apply.  Only the arg-max position contributes to dgamma / dbeta.
// Traffic per layer in units of the conv output: forward 1.375 instead of 3.25, backward 3.75 instead of 7.25.
// ------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void bn_leaky_pool_kernel(const T *__restrict__ Y, const float *__restrict__ mean, const float *__restrict__ var,
                                                            const float *__restrict__ gamma, const float *__restrict__ beta, T *__restrict__ P,
                                                            unsigned char *__restrict__ idx, int B, int H, int W, int C, int ldp, float eps, float alpha) {
    constexpr int N = Vec16<T>::N;
    RowMap rm(C, N);
    if (!rm.active) return;
    float mu[N], sc[N], bt[N];
#pragma unroll
    for (int j = 0; j < N; ++j) {
        int c = rm.cg * N + j;
        mu[j] = mean[c];
        sc[j] = bn_inv_std(var[c], eps) * gamma[c];
        bt[j] = beta[c];
    }
    const PoolRow pr(H, W, C);
    const long MP = (long)B * pr.OH * pr.OW;
    for (long r = (long)blockIdx.x * rm.rpp + rm.rs; r < MP; r += (long)gridDim.x * rm.rpp) {
        const T *src = Y + pr.base(r) + rm.cg * N;
        Vec16<T> v[4], o;
        v[0] = ld16(src);
        v[1] = ld16(src + C);
        v[2] = ld16(src + (long)W * C);
        v[3] = ld16(src + (long)W * C + C);
        typename IdxPack<N>::type pack = 0;
#pragma unroll
        for (int j = 0; j < N; ++j) {
            float a[4], m;
#pragma unroll
            for (int k = 0; k < 4; ++k) a[k] = pool_round<T>(bn_leaky(v[k].get(j), mu[j], sc[j], bt[j], alpha));
            const int arg = pool_first_max(a, m);
            o.set(j, m);
            pack |= idx_pack_byte<N>(arg, j);
        }
        st16(P + r * ldp + rm.cg * N, o);
        if (idx) *reinterpret_cast<typename IdxPack<N>::type *>(idx + r * C + rm.cg * N) = pack;
    }
}

template <typename T>
__global__ __launch_bounds__(256) void bn_pool_bwd_reduce_kernel(const T *__restrict__ dP, int lddp, const unsigned char *__restrict__ idx, const T *__restrict__ Y,
                                                                 const float *__restrict__ mean, const float *__restrict__ var, const float *__restrict__ gamma,
                                                                 const float *__restrict__ beta, float *__restrict__ ws, int B, int H, int W, int C, float eps, float alpha) {
    constexpr int N = Vec16<T>::N;
    RowMap rm(C, N);
    float part[2][N];
    float mu[N], inv[N], ga[N], bt[N];
#pragma unroll
    for (int j = 0; j < N; ++j) {
        part[0][j] = part[1][j] = 0.f;
        int c = rm.cg * N + j;
        bool ok = rm.active;
        mu[j] = ok ? mean[c] : 0.f;
        inv[j] = ok ? bn_inv_std(var[c], eps) : 0.f;
        ga[j] = ok ? gamma[c] : 0.f;
        bt[j] = ok ? beta[c] : 0.f;
    }
    if (rm.active) {
        const PoolRow pr(H, W, C);
        const long MP = (long)B * pr.OH * pr.OW;
        for (long r = (long)blockIdx.x * rm.rpp + rm.rs; r < MP; r += (long)gridDim.x * rm.rpp) {
            const T *src = Y + pr.base(r) + rm.cg * N;
            Vec16<T> v[4];
            v[0] = ld16(src);
            v[1] = ld16(src + C);
            v[2] = ld16(src + (long)W * C);
            v[3] = ld16(src + (long)W * C + C);
            const Vec16<T> d = ld16(dP + r * lddp + rm.cg * N);
            const typename IdxPack<N>::type pack = *reinterpret_cast<const typename IdxPack<N>::type *>(idx + r * C + rm.cg * N);
#pragma unroll
            for (int j = 0; j < N; ++j) {
                const int k = idx_pack_get(pack, j);
                const float y = k == 0 ? v[0].get(j) : k == 1 ? v[1].get(j) : k == 2 ? v[2].get(j) : v[3].get(j);
                const float xh = (y - mu[j]) * inv[j];      // bn_leaky.h bn_leaky_bwd, spelled out (the helper restructures this kernel)
                const float z = (y - mu[j]) * (inv[j] * ga[j]) + bt[j];
                const float g = z >= 0.f ? d.get(j) : alpha * d.get(j);
                part[0][j] += g * xh;
                part[1][j] += g;
            }
        }
    }
    block_colsum_store<N, 2>(part, rm, C, ws, gridDim.x);
}

template <typename T>
__global__ __launch_bounds__(256) void bn_pool_bwd_apply_kernel(const T *__restrict__ dP, int lddp, const unsigned char *__restrict__ idx, const T *__restrict__ Y,
                                                                const float *__restrict__ mean, const float *__restrict__ var, const float *__restrict__ gamma,
                                                                const float *__restrict__ beta, const float *__restrict__ dgamma, const float *__restrict__ dbeta,
                                                                T *__restrict__ dY, int B, int H, int W, int C, float eps, float alpha) {
    constexpr int N = Vec16<T>::N;
    RowMap rm(C, N);
    if (!rm.active) return;
    const float invM = 1.0f / (float)((long)B * H * W);
    float mu[N], inv[N], ga[N], bt[N], dgm[N], dbm[N];
#pragma unroll
    for (int j = 0; j < N; ++j) {
        int c = rm.cg * N + j;
        mu[j] = mean[c];
        inv[j] = bn_inv_std(var[c], eps);
        ga[j] = gamma[c];
        bt[j] = beta[c];
        dgm[j] = dgamma[c] * invM;
        dbm[j] = dbeta[c] * invM;
    }
    const PoolRow pr(H, W, C);
    const long MP = (long)B * pr.OH * pr.OW;
    for (long r = (long)blockIdx.x * rm.rpp + rm.rs; r < MP; r += (long)gridDim.x * rm.rpp) {
        const long off = pr.base(r) + rm.cg * N;
        const long koff[4] = {0, C, (long)W * C, (long)W * C + C};
        Vec16<T> v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = ld16(Y + off + koff[k]);
        const Vec16<T> d = ld16(dP + r * lddp + rm.cg * N);
        const typename IdxPack<N>::type pack = *reinterpret_cast<const typename IdxPack<N>::type *>(idx + r * C + rm.cg * N);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            Vec16<T> o;
#pragma unroll
            for (int j = 0; j < N; ++j) {
                const float da = pool_route(idx_pack_get(pack, j), k, d.get(j));
                o.set(j, bn_bwd_apply(bn_leaky_bwd(v[k].get(j), da, mu[j], inv[j], ga[j], bt[j], alpha), inv[j], ga[j], dgm[j], dbm[j]));
            }
            st16(dY + off + koff[k], o);
        }
    }
}

// ------------------------------------------------------------------------------------------
// Consumers that finalise the partial rows themselves (round 3): the 36 bn_finalize / 7 reduce_finalize launches of a training
// step were ~5 us each (a 16-workgroup kernel is all latency) plus a kernel boundary.  Here the kernel that NEEDS the batch
// moments (BN apply) or dgamma / dbeta (BN backward apply) sums the partial rows of its own channels in its prologue.
// Mapping: a workgroup owns ONE channel slice (blockIdx.y: up to 16 lanes x 16 bytes = 128 bf16 / 64 f32 channels) and strides
// over pixel rows (blockIdx.x), so its prologue reads rows x slice x 2 floats (L2-resident: the producer just wrote them) instead
// of rows x C x 2; the 256 threads split the rows, accumulate in f64, and meet in LDS.  The workgroups with blockIdx.x == 0 store
// mean / var (+ moving averages) or dgamma / dbeta for their slice.  Rows are read-only here: a buffer that needs to be zero for
// its next producer is cleared by the NEXT consumer kernel, which works on the other buffer of a pair (zero / zero_vec4 arguments).
// ------------------------------------------------------------------------------------------
struct SliceMap {   // 256 threads = rpb rows x lpr lanes; lane -> 16-byte channel group cg of slice blockIdx.y
    int lpr, rpb, lane, row, cg, cs, c0;
    __device__ SliceMap(int C, int vec) {
        const int tpr = C / vec;
        lpr = tpr < 16 ? tpr : 16;
        rpb = 256 / lpr;
        lane = threadIdx.x % lpr;
        row = threadIdx.x / lpr;
        cg = blockIdx.y * lpr + lane;
        cs = lpr * vec;                  // channels of the slice (<= 128)
        c0 = blockIdx.y * cs;
    }
};
#define Y2_SLICE_MAX 128

// thread c < cs: sums[k] = sum over rows of part[k * plane + row * C + c0 + c] (f64); ends with a barrier.  A thread owns four adjacent
// channels (one 16-byte load per row and plane) and every (256 / (cs / 4))-th row, so even a 128-channel slice has eight row groups
// working in parallel: the prologue is a dependent chain in front of the whole workgroup and its length is what the fold pays.
// the per-thread sums of the row groups that share a wave meet on the VALU (G = lanes per row: the lanes that share lane % G), then the four waves in LDS
template <int G>
__device__ __forceinline__ void slice_wave_sums(double (&v)[4]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = y2_lane_group_sum_f64<G>(v[j]);
}
__device__ __forceinline__ void slice_partial_sums(const float *__restrict__ part, int rows, long plane, int C, const SliceMap &sm, double (&sums)[2]) {
    // (round 6) 4 KB of scratch -- [wave][channel of the slice] per plane, one plane after the other -- and the results in registers of the threads that
    // use them (thread c < cs: sums[k] of channel c0 + c) instead of 16 + 2 KB: with < 8 KB of LDS these workgroups fit on a CU beside ANY
    // filter-gradient workgroup (140 .. 152 KB), which is where the side stream wants them
    __shared__ double red[4 * Y2_SLICE_MAX];
    const int q = sm.cs >> 2;                               // lanes per row (cs >= 8 for bf16, >= 4 for f32: q >= 1)
    const int l4 = threadIdx.x % q, g = threadIdx.x / q, ng = 256 / q;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool valu = q == 4 || q == 8 || q == 16 || q == 32;      // (q = 1, 2: tiny slices, the general path; 64 % q == 0 always)
    sums[0] = sums[1] = 0.0;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const float *p = part + (long)k * plane + sm.c0 + l4 * 4;
        // four independent 16-byte loads in flight per thread, the last group included (a row beyond the end loads row g again with weight 0): the
        // prologue is a chain of L2 latencies in front of the whole workgroup -- 44 rows over 8 row groups are two rounds instead of four
        double s[4] = {0.0, 0.0, 0.0, 0.0}, t[4] = {0.0, 0.0, 0.0, 0.0};
        for (int r = g; r < rows; r += 4 * ng) {
            f32x4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = *reinterpret_cast<const f32x4 *>(p + (long)(r + u * ng < rows ? r + u * ng : g) * C);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const bool ok = r + u * ng < rows;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const double x = ok ? (double)v[u][j] : 0.0;
                    if (u & 1) t[j] += x; else s[j] += x;
                }
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) s[j] += t[j];
        if (k) __syncthreads();                              // (plane 0's scratch has been read)
        if (valu) {
            if (q == 4) slice_wave_sums<4>(s); else if (q == 8) slice_wave_sums<8>(s); else if (q == 16) slice_wave_sums<16>(s); else slice_wave_sums<32>(s);
            if (lane < q) {
#pragma unroll
                for (int j = 0; j < 4; ++j) red[wave * sm.cs + lane * 4 + j] = s[j];
            }
            __syncthreads();
            if (threadIdx.x < sm.cs) sums[k] = (red[threadIdx.x] + red[sm.cs + threadIdx.x]) + (red[2 * sm.cs + threadIdx.x] + red[3 * sm.cs + threadIdx.x]);
        } else {
            // general path (slices of 4 or 8 channels: one or two lanes per row, 128 .. 256 row groups): through the same scratch in rounds of
            // 4 * Y2_SLICE_MAX / cs row groups
            const int gmax = 4 * Y2_SLICE_MAX / sm.cs;
            double a = 0.0;
            for (int g0 = 0; g0 < ng; g0 += gmax) {
                if (g0) __syncthreads();
                if (g >= g0 && g < g0 + gmax) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) red[(g - g0) * sm.cs + l4 * 4 + j] = s[j];
                }
                __syncthreads();
                if (threadIdx.x < sm.cs)
                    for (int j = 0; j < gmax && g0 + j < ng; ++j) a += red[j * sm.cs + threadIdx.x];
            }
            if (threadIdx.x < sm.cs) sums[k] = a;
        }
    }
    __syncthreads();
}

__device__ __forceinline__ void grid_zero(float *__restrict__ zero, long zero_vec4) {
    if (!zero) return;
    const long nthreads = (long)gridDim.x * gridDim.y * 256;
    f32x4 z = {0.f, 0.f, 0.f, 0.f};
    for (long i = ((long)blockIdx.y * gridDim.x + blockIdx.x) * 256 + threadIdx.x; i < zero_vec4; i += nthreads) reinterpret_cast<f32x4 *>(zero)[i] = z;
}

// forward: batch moments from the partial rows + BN apply + leaky (+ 2x2 max pool)
template <typename T, bool POOL>
__global__ __launch_bounds__(256) void bn_leaky_fin_kernel(const T *__restrict__ Y, const float *__restrict__ part, int rows, const float *__restrict__ shift,
                                                           long Mstat, float *__restrict__ mean_out, float *__restrict__ var_out, float *__restrict__ mm,
                                                           float *__restrict__ mv, float omd, const float *__restrict__ gamma, const float *__restrict__ beta,
                                                           T *__restrict__ A, unsigned char *__restrict__ idx, T *__restrict__ ymax, T *__restrict__ Afull,
                                                           int B, int H, int W, int C, int lda, float eps, float alpha, float *__restrict__ zero, long zero_vec4) {
    constexpr int N = Vec16<T>::N;
    const SliceMap sm(C, N);
    double sums[2];
    __shared__ float cst[3][Y2_SLICE_MAX];
    // the first pixel row's data is requested BEFORE the prologue: its HBM latency runs under the partial-row reduction
    const PoolRow pr(H, W, C);
    const long ML = POOL ? (long)B * pr.OH * pr.OW : (long)B * H * W;
    const long step = (long)gridDim.x * sm.rpb;
    long r = (long)blockIdx.x * sm.rpb + sm.row;
    Vec16<T> v[POOL ? 4 : 1];
    if (r < ML) {
        if (POOL) {
            const T *src = Y + pr.base(r) + sm.cg * N;
            v[0] = ld16(src);
            v[POOL ? 1 : 0] = ld16(src + C);
            v[POOL ? 2 : 0] = ld16(src + (long)W * C);
            v[POOL ? 3 : 0] = ld16(src + (long)W * C + C);
        } else v[0] = ld16(Y + r * C + sm.cg * N);
    }
    slice_partial_sums(part, rows, (long)Y2_BN_PART_ROWS * C, C, sm, sums);
    if (threadIdx.x < sm.cs) {
        const int c = sm.c0 + threadIdx.x;
        // the same arithmetic as bn_finalize_kernel<0> / reduce_finalize_kernel<0>, spelled out in all three: a shared helper changes those two kernels
        const double dm = sums[0] / (double)Mstat;
        const double var = sums[1] / (double)Mstat - dm * dm;
        const float fm = (float)((double)shift[c] + dm), fv = (float)(var > 0.0 ? var : 0.0);
        cst[0][threadIdx.x] = fm;
        cst[1][threadIdx.x] = bn_inv_std(fv, eps) * gamma[c];
        cst[2][threadIdx.x] = beta[c];
        if (blockIdx.x == 0) {
            mean_out[c] = fm;
            var_out[c] = fv;
            if (mm) {
                mm[c] = bn_ema(mm[c], fm, omd);
                mv[c] = bn_ema(mv[c], fv, omd);
            }
        }
    }
    __syncthreads();
    float mu[N], sc[N], bt[N];
#pragma unroll
    for (int j = 0; j < N; ++j) {
        mu[j] = cst[0][sm.lane * N + j];
        sc[j] = cst[1][sm.lane * N + j];
        bt[j] = cst[2][sm.lane * N + j];
    }
    grid_zero(zero, zero_vec4);
    while (r < ML) {
        const long rn = r + step;
        Vec16<T> vn[POOL ? 4 : 1];
        if (rn < ML) {       // next row in flight while this one is computed and stored
            if (POOL) {
                const T *src = Y + pr.base(rn) + sm.cg * N;
                vn[0] = ld16(src);
                vn[POOL ? 1 : 0] = ld16(src + C);
                vn[POOL ? 2 : 0] = ld16(src + (long)W * C);
                vn[POOL ? 3 : 0] = ld16(src + (long)W * C + C);
            } else vn[0] = ld16(Y + rn * C + sm.cg * N);
        }
        Vec16<T> o;
        if (!POOL) {
#pragma unroll
            for (int j = 0; j < N; ++j) o.set(j, bn_leaky(v[0].get(j), mu[j], sc[j], bt[j], alpha));
            st16(A + r * lda + sm.cg * N, o);
        } else {
            typename IdxPack<N>::type pack = 0;
            Vec16<T> ym, af[4];
#pragma unroll
            for (int j = 0; j < N; ++j) {
                float a[4], m;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    a[k] = pool_round<T>(bn_leaky(v[POOL ? k : 0].get(j), mu[j], sc[j], bt[j], alpha));
                    af[k].set(j, a[k]);
                }
                const int arg = pool_first_max(a, m);
                o.set(j, m);
                ym.set(j, arg == 0 ? v[0].get(j) : arg == 1 ? v[POOL ? 1 : 0].get(j) : arg == 2 ? v[POOL ? 2 : 0].get(j) : v[POOL ? 3 : 0].get(j));
                pack |= idx_pack_byte<N>(arg, j);
            }
            st16(A + r * lda + sm.cg * N, o);
            if (idx) *reinterpret_cast<typename IdxPack<N>::type *>(idx + r * C + sm.cg * N) = pack;
            if (Afull) {       // the activation has another reader besides the pool (Darknet-19's passthrough at the 26x26 stage): dense [B][H][W][C]
                T *dst = Afull + pr.base(r) + sm.cg * N;
                st16(dst, af[0]);
                st16(dst + C, af[1]);
                st16(dst + (long)W * C, af[2]);
                st16(dst + (long)W * C + C, af[3]);
            }
            if (ymax) st16(ymax + r * C + sm.cg * N, ym);       // the raw convolution output at the arg-max (the backward reduction reads this, not Y)
        }
#pragma unroll
        for (int k = 0; k < (POOL ? 4 : 1); ++k) v[k] = vn[k];
        r = rn;
    }
}

// backward: dgamma / dbeta from the partial rows (plain sums, as bn_finalize_kernel<1> / reduce_finalize_kernel<1>) + the apply pass
template <typename T, bool POOL>
__global__ __launch_bounds__(256) void bn_bwd_apply_fin_kernel(const T *__restrict__ dA, int ldda, const unsigned char *__restrict__ idx, const T *__restrict__ Y,
                                                               const float *__restrict__ mean, const float *__restrict__ var, const float *__restrict__ gamma,
                                                               const float *__restrict__ beta, const float *__restrict__ part, int rows, long plane,
                                                               float *__restrict__ dgamma, float *__restrict__ dbeta, T *__restrict__ dY, int B, int H, int W, int C,
                                                               float eps, float alpha, float *__restrict__ zero, long zero_vec4) {
    constexpr int N = Vec16<T>::N;
    const SliceMap sm(C, N);
    double sums[2];
    __shared__ float cst[2][Y2_SLICE_MAX];
    const PoolRow pr(H, W, C);
    const long ML = POOL ? (long)B * pr.OH * pr.OW : (long)B * H * W;
    const long step = (long)gridDim.x * sm.rpb;
    long r = (long)blockIdx.x * sm.rpb + sm.row;
    const long koff[4] = {0, C, (long)W * C, (long)W * C + C};
    Vec16<T> v[POOL ? 4 : 1], d;
    typename IdxPack<N>::type pack = 0;
    auto fetch = [&](long row, Vec16<T> (&yv)[POOL ? 4 : 1], Vec16<T> &dv, typename IdxPack<N>::type &pk) {
        if (POOL) {
            const long off = pr.base(row) + sm.cg * N;
#pragma unroll
            for (int k = 0; k < (POOL ? 4 : 1); ++k) yv[k] = ld16(Y + off + koff[k]);
            pk = *reinterpret_cast<const typename IdxPack<N>::type *>(idx + row * C + sm.cg * N);
        } else yv[0] = ld16(Y + row * C + sm.cg * N);
        dv = ld16(dA + row * ldda + sm.cg * N);
    };
    if (r < ML) fetch(r, v, d, pack);        // in flight under the prologue
    slice_partial_sums(part, rows, plane, C, sm, sums);
    if (threadIdx.x < sm.cs) {
        const float dg = (float)sums[0], db = (float)sums[1];
        cst[0][threadIdx.x] = dg;
        cst[1][threadIdx.x] = db;
        if (blockIdx.x == 0) {
            dgamma[sm.c0 + threadIdx.x] = dg;
            dbeta[sm.c0 + threadIdx.x] = db;
        }
    }
    __syncthreads();
    const float invM = 1.0f / (float)((long)B * H * W);
    float mu[N], inv[N], ga[N], bt[N], dgm[N], dbm[N];
#pragma unroll
    for (int j = 0; j < N; ++j) {
        const int c = sm.cg * N + j;
        mu[j] = mean[c];
        inv[j] = bn_inv_std(var[c], eps);
        ga[j] = gamma[c];
        bt[j] = beta[c];
        dgm[j] = cst[0][sm.lane * N + j] * invM;
        dbm[j] = cst[1][sm.lane * N + j] * invM;
    }
    grid_zero(zero, zero_vec4);
    while (r < ML) {
        const long rn = r + step;
        Vec16<T> vn[POOL ? 4 : 1], dn;
        typename IdxPack<N>::type packn = 0;
        if (rn < ML) fetch(rn, vn, dn, packn);
        if (!POOL) {
            Vec16<T> o;
#pragma unroll
            for (int j = 0; j < N; ++j) {      // (spelled out as in bn_bwd_apply_kernel)
                float xh = (v[0].get(j) - mu[j]) * inv[j];
                float z = (v[0].get(j) - mu[j]) * (inv[j] * ga[j]) + bt[j];
                float g = z >= 0.f ? d.get(j) : alpha * d.get(j);
                o.set(j, (ga[j] * inv[j]) * (g - dbm[j] - xh * dgm[j]));
            }
            st16(dY + r * C + sm.cg * N, o);
        } else {
            const long off = pr.base(r) + sm.cg * N;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                Vec16<T> o;
#pragma unroll
                for (int j = 0; j < N; ++j) {
                    const float da = pool_route(idx_pack_get(pack, j), k, d.get(j));
                    o.set(j, bn_bwd_apply(bn_leaky_bwd(v[POOL ? k : 0].get(j), da, mu[j], inv[j], ga[j], bt[j], alpha), inv[j], ga[j], dgm[j], dbm[j]));
                }
                st16(dY + off + koff[k], o);
            }
        }
#pragma unroll
        for (int k = 0; k < (POOL ? 4 : 1); ++k) v[k] = vn[k];
        d = dn;
        pack = packn;
        r = rn;
    }
}

// ---- fused BN + leaky + max pool entry points
static bool pool_args_ok(int B, int H, int W, int C, int dtype) {
    const int vec = dtype == YOLO2_BF16 ? 8 : 4;
    return B > 0 && H > 0 && W > 0 && C > 0 && H % 2 == 0 && W % 2 == 0 && C % vec == 0 && C / vec <= 256;
}
extern "C" int yolo2_bn_leaky_pool(const void *Y, const float *mean, const float *var, const float *gamma, const float *beta, void *P,
                                   unsigned char *idx, int B, int H, int W, int C, int ldp, float eps, float alpha, int dtype, void *stream) {
    Y2_CHECK_ARG(Y && mean && var && gamma && beta && P && ldp >= C);
    Y2_CHECK_ARG(pool_args_ok(B, H, W, C, dtype) && ldp % (dtype == YOLO2_BF16 ? 8 : 4) == 0);
    const int vec = dtype == YOLO2_BF16 ? 8 : 4;
    const long MP = (long)B * (H / 2) * (W / 2);
    int grid = rowmap_grid(MP, C, vec, 2);
    Y2_DISPATCH_DTYPE(dtype, bn_leaky_pool_kernel<T><<<grid, 256, 0, (hipStream_t)stream>>>((const T *)Y, mean, var, gamma, beta, (T *)P, idx, B, H, W, C, ldp, eps, alpha));
    Y2_CHECK_LAUNCH();
    return YOLO2_OK;
}
static int pool_bwd_reduce_impl(const void *dP, int lddp, const unsigned char *idx, const void *Y, const float *mean, const float *var,
                                const float *gamma, const float *beta, float *dgamma, float *dbeta, double *ws, int *rows, int rows_limit, int B, int H, int W,
                                int C, float eps, float alpha, int dtype, void *stream) {
    Y2_CHECK_ARG(dP && idx && Y && mean && var && gamma && beta && ws && lddp >= C);
    Y2_CHECK_ARG(pool_args_ok(B, H, W, C, dtype));
    const int vec = dtype == YOLO2_BF16 ? 8 : 4;
    hipStream_t st = (hipStream_t)stream;
    const long MP = (long)B * (H / 2) * (W / 2);
    int nb = colsum_grid(MP, C, vec);
    // the 416x416 / 208x208 stages (> 64 MB of conv output): one workgroup per CU is latency-bound at 3 TB/s (measured 80 -> 62 us
    // with four); smaller tensors keep the short finalisation
    const int big = 1024;
    if (big > nb && (long)B * H * W * C * (16 / vec) >= (64L << 20)) {
        const int tpr = C / vec, rpp = 256 / tpr < 1 ? 1 : 256 / tpr;
        long g = (MP + (long)rpp * 4 - 1) / ((long)rpp * 4);
        nb = (int)(g < big ? g : big);
        if (nb > 1024) nb = 1024;
    }
    if (nb > rows_limit) nb = rows_limit;
    float *part = (float *)ws;
    Y2_DISPATCH_DTYPE(dtype, bn_pool_bwd_reduce_kernel<T><<<nb, 256, 0, st>>>((const T *)dP, lddp, idx, (const T *)Y, mean, var, gamma, beta, part, B, H, W, C, eps, alpha));
    if (rows) *rows = nb;
    else reduce_finalize_kernel<1><<<cdiv(C, 16), 256, 0, st>>>(part, nb, C, (long)B * H * W, dgamma, dbeta, C);
    Y2_CHECK_LAUNCH();
    return YOLO2_OK;
}
extern "C" int yolo2_bn_leaky_pool_bwd_reduce(const void *dP, int lddp, const unsigned char *idx, const void *Y, const float *mean, const float *var,
                                              const float *gamma, const float *beta, float *dgamma, float *dbeta, double *ws, int B, int H, int W,
                                              int C, float eps, float alpha, int dtype, void *stream) {
    Y2_CHECK_ARG(dgamma && dbeta);
    return pool_bwd_reduce_impl(dP, lddp, idx, Y, mean, var, gamma, beta, dgamma, dbeta, ws, nullptr, 1024, B, H, W, C, eps, alpha, dtype, stream);
}
// reduction alone: partial rows [2][*rows][C] stay in ws (for yolo2_bn_leaky_pool_bwd_apply_fin); at most rows_limit of them
extern "C" int yolo2_bn_leaky_pool_bwd_reduce_part(const void *dP, int lddp, const unsigned char *idx, const void *Y, const float *mean, const float *var,
                                                   const float *gamma, const float *beta, double *ws, int *rows, int rows_limit, int B, int H, int W, int C,
                                                   float eps, float alpha, int dtype, void *stream) {
    Y2_CHECK_ARG(rows && rows_limit >= 1);
    return pool_bwd_reduce_impl(dP, lddp, idx, Y, mean, var, gamma, beta, nullptr, nullptr, ws, rows, rows_limit, B, H, W, C, eps, alpha, dtype, stream);
}
extern "C" int yolo2_bn_leaky_pool_bwd_apply(const void *dP, int lddp, const unsigned char *idx, const void *Y, const float *mean, const float *var,
                                             const float *gamma, const float *beta, const float *dgamma, const float *dbeta, void *dY, int B, int H,
                                             int W, int C, float eps, float alpha, int dtype, void *stream) {
    Y2_CHECK_ARG(dP && idx && Y && mean && var && gamma && beta && dgamma && dbeta && dY && lddp >= C);
    Y2_CHECK_ARG(pool_args_ok(B, H, W, C, dtype));
    const int vec = dtype == YOLO2_BF16 ? 8 : 4;
    const long MP = (long)B * (H / 2) * (W / 2);
    int grid = rowmap_grid(MP, C, vec, 2);
    Y2_DISPATCH_DTYPE(dtype, bn_pool_bwd_apply_kernel<T><<<grid, 256, 0, (hipStream_t)stream>>>((const T *)dP, lddp, idx, (const T *)Y, mean, var, gamma, beta, dgamma, dbeta, (T *)dY, B, H, W, C, eps, alpha));
    Y2_CHECK_LAUNCH();
    return YOLO2_OK;
}

// ---- consumers with the finalisation in their prologue (kernels: bn_leaky_fin_kernel, bn_bwd_apply_fin_kernel)
static bool fin_shape_ok(int rows, int C, int dtype) {
    const int vec = dtype == YOLO2_BF16 ? 8 : 4;
    if (rows < 1 || C < vec || C % vec) return false;
    const int tpr = C / vec;
    if (tpr & (tpr - 1)) return false;                       // lanes per row must divide 256
    const int lpr = tpr < 16 ? tpr : 16;
    return (long)rows * lpr * vec * 8 <= (128L << 10);      // the prologue of EVERY workgroup reads this much: beyond it a separate finalisation is cheaper
}
extern "C" int yolo2_bn_fin_supported(int rows, int C, int dtype) { return fin_shape_ok(rows, C, dtype) ? 1 : 0; }

static dim3 slice_grid(long loop_rows, int C, int vec, int rows_per_thread, int part_rows) {
    const int tpr = C / vec, lpr = tpr < 16 ? tpr : 16, rpb = 256 / lpr, slices = tpr / lpr;
    long gx = (loop_rows + (long)rpb * rows_per_thread - 1) / ((long)rpb * rows_per_thread);
    const long per = (long)part_rows * lpr * vec * 8;        // prologue bytes per workgroup
    long cap = (48L << 20) / (per * slices);                 // <= ~48 MB of L2 reads for all prologues together ...
    const long floor_ = (512 + slices - 1) / slices;         // ... but never fewer than two workgroups per CU
    if (cap < floor_) cap = floor_;
    if (cap > 4096 / slices) cap = 4096 / slices;
    if (gx > cap) gx = cap;
    if (gx < 1) gx = 1;
    return dim3((unsigned)gx, (unsigned)slices);
}
#define Y2_CHECK_ZERO(zero, zero_floats) Y2_CHECK_ARG((zero_floats) >= 0 && (zero_floats) % 4 == 0 && ((zero) || (zero_floats) == 0) && ((uintptr_t)(zero) & 15) == 0)

extern "C" int yolo2_bn_leaky_fin(const void *Y, const float *bn_part, int rows, const float *shift, float *mean, float *var, float *moving_mean,
                                  float *moving_var, double decay, const float *gamma, const float *beta, void *A, long M, int C, int lda, float eps,
                                  float alpha, float *zero, long zero_floats, int dtype, void *stream) {
    Y2_CHECK_ARG(Y && bn_part && shift && mean && var && gamma && beta && A && M > 0 && C > 0 && lda >= C && M < (1L << 31));
    Y2_CHECK_ARG((moving_mean == nullptr) == (moving_var == nullptr) && rows <= Y2_BN_PART_ROWS && fin_shape_ok(rows, C, dtype));
    Y2_CHECK_ARG(shift != moving_mean && shift != mean);      // every workgroup reads the shift; one per channel slice writes these (see the header)
    Y2_CHECK_ZERO(zero, zero_floats);
    const int vec = dtype == YOLO2_BF16 ? 8 : 4;
    Y2_CHECK_ARG(lda % vec == 0);
    const dim3 grid = slice_grid(M, C, vec, 4, rows);
    Y2_DISPATCH_DTYPE(dtype, bn_leaky_fin_kernel<T, false><<<grid, 256, 0, (hipStream_t)stream>>>((const T *)Y, bn_part, rows, shift, M, mean, var, moving_mean, moving_var,
                      (float)(1.0 - decay), gamma, beta, (T *)A, nullptr, nullptr, nullptr, 1, 1, (int)M, C, lda, eps, alpha, zero, zero_floats / 4));
    Y2_CHECK_LAUNCH();
    return YOLO2_OK;
}

extern "C" int yolo2_bn_leaky_pool_fin(const void *Y, const float *bn_part, int rows, const float *shift, float *mean, float *var, float *moving_mean,
                                       float *moving_var, double decay, const float *gamma, const float *beta, void *P, unsigned char *idx, void *ymax,
                                       void *A_full, int B, int H, int W, int C, int ldp, float eps, float alpha, float *zero, long zero_floats, int dtype,
                                       void *stream) {
    Y2_CHECK_ARG(Y && bn_part && shift && mean && var && gamma && beta && P && ldp >= C);
    Y2_CHECK_ARG(pool_args_ok(B, H, W, C, dtype) && ldp % (dtype == YOLO2_BF16 ? 8 : 4) == 0);
    Y2_CHECK_ARG((moving_mean == nullptr) == (moving_var == nullptr) && rows <= Y2_BN_PART_ROWS && fin_shape_ok(rows, C, dtype));
    Y2_CHECK_ARG(shift != moving_mean && shift != mean);
    Y2_CHECK_ZERO(zero, zero_floats);
    const int vec = dtype == YOLO2_BF16 ? 8 : 4;
    const dim3 grid = slice_grid((long)B * (H / 2) * (W / 2), C, vec, 2, rows);
    Y2_DISPATCH_DTYPE(dtype, bn_leaky_fin_kernel<T, true><<<grid, 256, 0, (hipStream_t)stream>>>((const T *)Y, bn_part, rows, shift, (long)B * H * W, mean, var, moving_mean,
                      moving_var, (float)(1.0 - decay), gamma, beta, (T *)P, idx, (T *)ymax, (T *)A_full, B, H, W, C, ldp, eps, alpha, zero, zero_floats / 4));
    Y2_CHECK_LAUNCH();
    return YOLO2_OK;
}

extern "C" int yolo2_bn_leaky_bwd_apply_fin(const void *dA, int ldda, const void *Y, const float *mean, const float *var, const float *gamma, const float *beta,
                                            const float *part, int rows, long plane_stride, float *dgamma, float *dbeta, void *dY, long M, int C, float eps,
                                            float alpha, float *zero, long zero_floats, int dtype, void *stream) {
    Y2_CHECK_ARG(dA && Y && mean && var && gamma && beta && part && dgamma && dbeta && dY && M > 0 && C > 0 && ldda >= C && M < (1L << 31));
    Y2_CHECK_ARG(plane_stride >= (long)rows * C && fin_shape_ok(rows, C, dtype));
    Y2_CHECK_ZERO(zero, zero_floats);
    const int vec = dtype == YOLO2_BF16 ? 8 : 4;
    Y2_CHECK_ARG(ldda % vec == 0);
    const dim3 grid = slice_grid(M, C, vec, 4, rows);
    Y2_DISPATCH_DTYPE(dtype, bn_bwd_apply_fin_kernel<T, false><<<grid, 256, 0, (hipStream_t)stream>>>((const T *)dA, ldda, nullptr, (const T *)Y, mean, var, gamma, beta, part, rows,
                      plane_stride, dgamma, dbeta, (T *)dY, 1, 1, (int)M, C, eps, alpha, zero, zero_floats / 4));
    Y2_CHECK_LAUNCH();
    return YOLO2_OK;
}

extern "C" int yolo2_bn_leaky_pool_bwd_apply_fin(const void *dP, int lddp, const unsigned char *idx, const void *Y, const float *mean, const float *var,
                                                 const float *gamma, const float *beta, const float *part, int rows, long plane_stride, float *dgamma,
                                                 float *dbeta, void *dY, int B, int H, int W, int C, float eps, float alpha, float *zero, long zero_floats,
                                                 int dtype, void *stream) {
    Y2_CHECK_ARG(dP && idx && Y && mean && var && gamma && beta && part && dgamma && dbeta && dY && lddp >= C);
    Y2_CHECK_ARG(pool_args_ok(B, H, W, C, dtype) && plane_stride >= (long)rows * C && fin_shape_ok(rows, C, dtype));
    Y2_CHECK_ZERO(zero, zero_floats);
    const int vec = dtype == YOLO2_BF16 ? 8 : 4;
    const dim3 grid = slice_grid((long)B * (H / 2) * (W / 2), C, vec, 2, rows);
    Y2_DISPATCH_DTYPE(dtype, bn_bwd_apply_fin_kernel<T, true><<<grid, 256, 0, (hipStream_t)stream>>>((const T *)dP, lddp, idx, (const T *)Y, mean, var, gamma, beta, part, rows,
                      plane_stride, dgamma, dbeta, (T *)dY, B, H, W, C, eps, alpha, zero, zero_floats / 4));
    Y2_CHECK_LAUNCH();
    return YOLO2_OK;
}

// the reduction halves of yolo2_bn_leaky_bwd_reduce / yolo2_bn_leaky_pool_bwd_reduce alone: partial rows [2][*rows][C] left in ws for a *_fin consumer
extern "C" int yolo2_bn_leaky_bwd_reduce_part(const void *dA, int ldda, const void *Y, const float *mean, const float *var, const float *gamma,
                                              const float *beta, double *ws, int *rows, int rows_limit, long M, int C, float eps, float alpha, int dtype,
                                              void *stream) {
    Y2_CHECK_ARG(dA && Y && mean && var && gamma && beta && ws && rows && rows_limit >= 1 && M > 0 && C > 0 && ldda >= C);
    const int vec = dtype == YOLO2_BF16 ? 8 : 4;
    Y2_CHECK_ARG(C % vec == 0 && C / vec <= 256 && ldda % vec == 0);
    int nb = colsum_grid(M, C, vec);
    // > 32 MB to read (the pooled 208x208 / 104x104 stages): one workgroup per CU is latency-bound, as for the pooled reduction above
    const int big = 1024;
    if (big > nb && M * C * (16 / vec) * 2 >= (32L << 20)) {
        const int tpr = C / vec, rpp = 256 / tpr < 1 ? 1 : 256 / tpr;
        const long g = (M + (long)rpp * 16 - 1) / ((long)rpp * 16);
        nb = (int)(g < big ? g : big);
        if (nb > 1024) nb = 1024;
    }
    if (nb > rows_limit) nb = rows_limit;
    Y2_DISPATCH_DTYPE(dtype, bn_bwd_reduce_kernel<T><<<nb, 256, 0, (hipStream_t)stream>>>((const T *)dA, ldda, (const T *)Y, mean, var, gamma, beta, (float *)ws, M, C, eps, alpha));
    Y2_CHECK_LAUNCH();
    *rows = nb;
    return YOLO2_OK;
}
