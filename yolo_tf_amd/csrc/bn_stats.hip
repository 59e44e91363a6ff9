// Batch-norm statistics, bias gradient and the sums of a fused BN backward (gfx950): column sums over [M][C] as partial rows per workgroup, finalised in f64.
#include "common.h"
#include "bn_leaky.h"
#include "colsum.h"

// K = 2: single-pass moments, SHIFTED by the channel's first sample s = X[0][c]: the partials are
// sum (x-s) and sum (x-s)^2, so the f64 finalisation's E[d^2] - E[d]^2 cancels against (mean-s)^2 ~ var
// instead of mean^2 (plain E[x^2]-mean^2 loses the variance when |mean| >> std, e.g. few samples per
// channel).  Block 0 also stores s as a third row of the partial buffer.   K = 1: plain column sum.
template <typename T, int K>
__global__ __launch_bounds__(256) void colsum_kernel(const T *__restrict__ X, int ld, long M, int C, float *__restrict__ part,
                                                     const float *__restrict__ shift_in = nullptr, int nb_rows = 0) {
    constexpr int N = Vec16<T>::N;
    RowMap rm(C, N);
    float acc[K][N], sh[N];
#pragma unroll
    for (int j = 0; j < N; ++j) sh[j] = 0.f;
    if (K == 2 && rm.active && shift_in) {
#pragma unroll
        for (int j = 0; j < N; ++j) sh[j] = shift_in[rm.cg * N + j];
    } else if (K == 2 && rm.active) {
        Vec16<T> v0 = ld16(X + rm.cg * N);
#pragma unroll
        for (int j = 0; j < N; ++j) sh[j] = v0.get(j);
        if (blockIdx.x == 0 && rm.rs == 0)
#pragma unroll
            for (int j = 0; j < N; ++j) part[(long)2 * gridDim.x * C + rm.cg * N + j] = sh[j];
    }
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
        for (int j = 0; j < N; ++j) acc[k][j] = 0.f;
    if (rm.active) {
        const long step = (long)gridDim.x * rm.rpp;
        long r = (long)blockIdx.x * rm.rpp + rm.rs;
        for (; r + 3 * step < M; r += 4 * step) {          // 4 independent 16-byte loads in flight per lane
            Vec16<T> v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = ld16(X + (r + u * step) * ld + rm.cg * N);
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int j = 0; j < N; ++j) {
                    float x = v[u].get(j) - sh[j];
                    acc[0][j] += x;
                    if (K == 2) acc[K - 1][j] += x * x;
                }
        }
        for (; r < M; r += step) {
            Vec16<T> v = ld16(X + r * ld + rm.cg * N);
#pragma unroll
            for (int j = 0; j < N; ++j) {
                float x = v.get(j) - sh[j];
                acc[0][j] += x;
                if (K == 2) acc[K - 1][j] += x * x;
            }
        }
    }
    block_colsum_store<N, K>(acc, rm, C, part, nb_rows ? nb_rows : gridDim.x);
}

// Fallback producer of the convolution epilogue's partial format ([2][Y2_BN_PART_ROWS][C], zero on entry): used for the
// layers whose convolution cannot produce the sums itself (first-layer direct kernel, K-sliced grids).
int y2_colsum_rows(long M, int C, int dtype) {
    const int vec = dtype == YOLO2_BF16 ? 8 : 4;
    int nb = colsum_grid(M, C, vec);
    if (nb > Y2_BN_PART_ROWS) nb = Y2_BN_PART_ROWS;
    // no more rows than a consumer that finalises them in its prologue reads (bn.hip fin_shape_ok: rows x slice x 8 bytes <= 128 KB)
    const long lim = (128L << 10) / ((long)(C / vec < 16 ? C / vec : 16) * vec * 8);
    return nb > lim ? (int)lim : nb;
}
int y2_colsum_into(const void *Y, int ld, long M, int C, const float *shift, float *part, int dtype, hipStream_t st) {
    const int vec = dtype == YOLO2_BF16 ? 8 : 4;
    Y2_CHECK_ARG(C % vec == 0 && C / vec <= 256 && ld == C);
    const int nb = y2_colsum_rows(M, C, dtype);
    Y2_DISPATCH_DTYPE(dtype, colsum_kernel<T, 2><<<nb, 256, 0, st>>>((const T *)Y, ld, M, C, part, shift, Y2_BN_PART_ROWS));
    Y2_CHECK_LAUNCH();
    return YOLO2_OK;
}

// partial rows -> batch mean / biased variance (+ moving-average update), and the rows are zeroed again for the next step
template <int FIN>      // 0: batch moments (+ moving averages); 1: plain column sums (plane 0 -> mean_out, plane 1 -> var_out)
__global__ __launch_bounds__(256) void bn_finalize_kernel(float *__restrict__ part, const float *__restrict__ shift, int C, long M,
                                                          float *__restrict__ mean_out, float *__restrict__ var_out,
                                                          float *__restrict__ mm, float *__restrict__ mv, float omd) {
    constexpr int NB = Y2_BN_PART_ROWS;
    __shared__ double red[2][16][17];
    const int col = threadIdx.x & 15, rg = threadIdx.x >> 4;
    const int c = blockIdx.x * 16 + col;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
        if (c < C) {
            float *p = part + (long)k * NB * C + c;
            float v[NB / 16];
#pragma unroll
            for (int u = 0; u < NB / 16; ++u) v[u] = p[(long)(rg + 16 * u) * C];
#pragma unroll
            for (int u = 0; u < NB / 16; ++u) p[(long)(rg + 16 * u) * C] = 0.f;
#pragma unroll
            for (int u = 0; u < NB / 16; u += 4) {
                s0 += (double)v[u];
                s1 += (double)v[u + 1];
                s2 += (double)v[u + 2];
                s3 += (double)v[u + 3];
            }
        }
        red[k][rg][col] = (s0 + s1) + (s2 + s3);
    }
    __syncthreads();
    if (rg == 0 && c < C) {
        double t[2];
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            double a = 0.0;
#pragma unroll
            for (int r = 0; r < 16; ++r) a += red[k][r][col];
            t[k] = a;
        }
        if (FIN == 1) {
            mean_out[c] = (float)t[0];
            var_out[c] = (float)t[1];
            return;
        }
        const double dm = t[0] / (double)M;
        const double var = t[1] / (double)M - dm * dm;
        const double mean = (double)shift[c] + dm;
        const float fm = (float)mean, fv = (float)(var > 0.0 ? var : 0.0);
        mean_out[c] = fm;
        var_out[c] = fv;
        if (mm) {
            mm[c] = bn_ema(mm[c], fm, omd);
            mv[c] = bn_ema(mv[c], fv, omd);
        }
    }
}
extern "C" int yolo2_bn_finalize(float *bn_part, const float *shift, long M, int C, float *mean, float *var, float *moving_mean,
                                 float *moving_var, double decay, void *stream) {
    Y2_CHECK_ARG(bn_part && shift && mean && var && M > 0 && C > 0);
    Y2_CHECK_ARG((moving_mean == nullptr) == (moving_var == nullptr));
    bn_finalize_kernel<0><<<cdiv(C, 16), 256, 0, (hipStream_t)stream>>>(bn_part, shift, C, M, mean, var, moving_mean, moving_var, (float)(1.0 - decay));
    Y2_CHECK_LAUNCH();
    return YOLO2_OK;
}

int y2_bn_part_to_grads(float *part, int C, float *dgamma, float *dbeta, hipStream_t st) {
    bn_finalize_kernel<1><<<cdiv(C, 16), 256, 0, st>>>(part, nullptr, C, 1, dgamma, dbeta, nullptr, nullptr, 0.f);
    Y2_CHECK_LAUNCH();
    return YOLO2_OK;
}

static int bn_stats_impl(const void *Y, float *mean, float *var, float *mm, float *mv, double decay, double *ws, long M, int C, int dtype, void *stream) {
    Y2_CHECK_ARG(Y && mean && var && ws && M > 0 && C > 0);
    const int vec = dtype == YOLO2_BF16 ? 8 : 4;
    Y2_CHECK_ARG(C % vec == 0 && C / vec <= 256);
    hipStream_t st = (hipStream_t)stream;
    const int nb = colsum_grid(M, C, vec);
    float *part = (float *)ws;
    Y2_DISPATCH_DTYPE(dtype, colsum_kernel<T, 2><<<nb, 256, 0, st>>>((const T *)Y, C, M, C, part));
    reduce_finalize_kernel<0><<<cdiv(C, 16), 256, 0, st>>>(part, nb, C, M, mean, var, C, mm, mv, (float)(1.0 - decay));
    Y2_CHECK_LAUNCH();
    return YOLO2_OK;
}
extern "C" int yolo2_bn_stats(const void *Y, float *mean, float *var, double *ws, long M, int C, int dtype, void *stream) {
    return bn_stats_impl(Y, mean, var, nullptr, nullptr, 0.0, ws, M, C, dtype, stream);
}
extern "C" int yolo2_bn_stats_ema(const void *Y, float *mean, float *var, float *moving_mean, float *moving_var, double decay,
                                  double *ws, long M, int C, int dtype, void *stream) {
    Y2_CHECK_ARG(moving_mean && moving_var);
    return bn_stats_impl(Y, mean, var, moving_mean, moving_var, decay, ws, M, C, dtype, stream);
}

// wide rows (the fully connected layers of the YOLO v1 family: M = batch, thousands of columns): one lane per column, rows in order
template <typename T>
__global__ void colsum_wide_kernel(const T *__restrict__ dY, int ld, long M, int C, float *__restrict__ dbias) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    double acc = 0.0;
    for (long r = 0; r < M; ++r) acc += (double)(float)dY[r * ld + c];
    dbias[c] = (float)acc;
}

// few rows (the detection head: 13x13 cells x batch): ONE launch, a workgroup per 16-byte channel group; every thread sums every 256th
// row in f32 (a handful of rows), the 256 partials meet in f64 through LDS.  The two-stage form costs a second 5 us launch here.
template <typename T>
__global__ __launch_bounds__(256) void colsum_direct_kernel(const T *__restrict__ dY, int ld, long M, int C, float *__restrict__ dbias) {
    constexpr int N = Vec16<T>::N;
    const T *col = dY + (long)blockIdx.x * N;
    float acc[N];
#pragma unroll
    for (int j = 0; j < N; ++j) acc[j] = 0.f;
    long r = threadIdx.x;
    for (; r + 768 < M; r += 1024) {       // four independent 16-byte loads in flight
        Vec16<T> v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = ld16(col + (r + 256 * u) * ld);
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int j = 0; j < N; ++j) acc[j] += v[u].get(j);
    }
    for (; r < M; r += 256) {
        const Vec16<T> v = ld16(col + r * ld);
#pragma unroll
        for (int j = 0; j < N; ++j) acc[j] += v.get(j);
    }
    __shared__ double red[256][N + 1];
#pragma unroll
    for (int j = 0; j < N; ++j) red[threadIdx.x][j] = (double)acc[j];
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s)
#pragma unroll
            for (int j = 0; j < N; ++j) red[threadIdx.x][j] += red[threadIdx.x + s][j];
        __syncthreads();
    }
    const int c = blockIdx.x * N + threadIdx.x;
    if ((int)threadIdx.x < N && c < C) dbias[c] = (float)red[0][threadIdx.x];
}

extern "C" int yolo2_bias_grad(const void *dY, int ld, float *dbias, double *ws, long M, int C, int dtype, void *stream) {
    Y2_CHECK_ARG(dY && dbias && ws && M > 0 && C > 0 && ld >= C);
    const int vec = dtype == YOLO2_BF16 ? 8 : 4;
    hipStream_t st = (hipStream_t)stream;
    if (ld / vec > 256) {
        Y2_CHECK_ARG(M <= 4096);
        Y2_DISPATCH_DTYPE(dtype, colsum_wide_kernel<T><<<cdiv(C, 256), 256, 0, st>>>((const T *)dY, ld, M, C, dbias));
        Y2_CHECK_LAUNCH();
        return YOLO2_OK;
    }
    Y2_CHECK_ARG(ld % vec == 0);
    const long direct_rows = 8192;
    if (M <= direct_rows && ((uintptr_t)dY & 15) == 0) {
        Y2_DISPATCH_DTYPE(dtype, colsum_direct_kernel<T><<<cdiv(C, vec), 256, 0, st>>>((const T *)dY, ld, M, C, dbias));
        Y2_CHECK_LAUNCH();
        return YOLO2_OK;
    }
    // reduce over the padded width ld (padding lanes are zero by contract), report the first C
    const int nb = colsum_grid(M, ld, vec);
    float *part = (float *)ws;
    Y2_DISPATCH_DTYPE(dtype, colsum_kernel<T, 1><<<nb, 256, 0, st>>>((const T *)dY, ld, M, ld, part));
    reduce_finalize_kernel<2><<<cdiv(ld, 16), 256, 0, st>>>(part, nb, ld, M, dbias, nullptr, C);
    Y2_CHECK_LAUNCH();
    return YOLO2_OK;
}

__global__ void bn_ema_kernel(float *mm, float *mv, const float *mean, const float *var, int C, float one_minus_decay) {
    int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < C) {
        mm[c] = bn_ema(mm[c], mean[c], one_minus_decay);
        mv[c] = bn_ema(mv[c], var[c], one_minus_decay);
    }
}
extern "C" int yolo2_bn_ema(float *moving_mean, float *moving_var, const float *mean, const float *var, int C, double decay, void *stream) {
    Y2_CHECK_ARG(moving_mean && moving_var && mean && var && C > 0);
    bn_ema_kernel<<<cdiv(C, 256), 256, 0, (hipStream_t)stream>>>(moving_mean, moving_var, mean, var, C, (float)(1.0 - decay));
    Y2_CHECK_LAUNCH();
    return YOLO2_OK;
}

// ---- workspace sizes (bytes) of the caller-owned scratch of yolo2_bn_stats* / the BN-backward reductions (<= 1024 partial rows + the shift row) and yolo2_bias_grad
extern "C" size_t yolo2_bn_workspace_bytes(int C) { return (size_t)1025 * (size_t)(C > 0 ? C : 0) * sizeof(double); }
extern "C" size_t yolo2_bias_grad_workspace_bytes(int ld) { return (size_t)512 * (size_t)(ld > 0 ? ld : 0) * sizeof(double); }
