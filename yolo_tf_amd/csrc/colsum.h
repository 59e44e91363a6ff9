// Column reductions over [M][C] (pixel stride ld) shared by bn_stats.hip and the BN-backward reductions of bn.hip: thread map, block reduction, grid rule, finalisation.
#pragma once
#include "common.h"
#include "bn_leaky.h"

struct RowMap {  // fixed channel group per thread, rows strided
    int tpr, rpp, cg, rs;
    bool active;
    __device__ RowMap(int C, int vec) {
        tpr = C / vec;
        rpp = 256 / tpr;
        if (rpp < 1) rpp = 1;
        cg = threadIdx.x % tpr;
        rs = threadIdx.x / tpr;
        active = rs < rpp && threadIdx.x < tpr * rpp;
    }
};

// Column reductions are two-stage and atomic-free: every block reduces its row slots through LDS
// and stores one f32 partial per (quantity, channel) at part[(k*nb + block)*C + c]; a second kernel
// sums the nb partials per channel in f64 and applies the finalisation (mean/var, dgamma/dbeta,
// bias gradient).  (A first version used f64 atomics on 2*C addresses: 2048 blocks contending on
// 64 addresses made the reductions 40 % of the training step.)
// (round 6) With 4 .. 32 threads per row -- 32 .. 256 channels in bf16 -- the row slots of a wave meet on the VALU first (common.h y2_lane_group_sum: the
// lanes that share lane % tpr) and only the four waves' sums go through LDS.  The general path below leaves the whole sum to `tpr` threads, rpp serial
// LDS reads per value: with 32 channels that is 4 threads x 1024 dependent reads, ~15 us at the end of every launch (measured: conv0's BN-backward
// reduction took 33 us for 88 MB, its 128-channel sibling 19 us for 22 MB).
// One 8 KB scratch for every form of the block reduction below (a __shared__ array inside a function template is allocated once per instantiation:
// the four lane-group forms + the general path had grown the BN-backward reduction's workgroups to 48 KB of LDS)
__device__ __forceinline__ float *colsum_scratch() {
    __shared__ float buf[2048];
    return buf;
}
template <int N, int K, int G>
__device__ __forceinline__ void block_colsum_store_g(const float (&part)[K][N], int C, float *out, int nb) {
    float *const redw = colsum_scratch();      // [quantity][wave][channel group][value]: K x 4 x 32 x N floats <= 8 KB
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
        for (int j = 0; j < N; ++j) {
            const float v = y2_lane_group_sum<G>(part[k][j]);
            if (lane < G) redw[((k * 4 + wave) * 32 + lane) * N + j] = v;
        }
    __syncthreads();
    if (threadIdx.x < G) {
#pragma unroll
        for (int k = 0; k < K; ++k)
#pragma unroll
            for (int j = 0; j < N; ++j)
                out[((long)k * nb + blockIdx.x) * C + threadIdx.x * N + j] =
                    (redw[((k * 4 + 0) * 32 + threadIdx.x) * N + j] + redw[((k * 4 + 1) * 32 + threadIdx.x) * N + j]) +
                    (redw[((k * 4 + 2) * 32 + threadIdx.x) * N + j] + redw[((k * 4 + 3) * 32 + threadIdx.x) * N + j]);
    }
}
template <int N, int K>
__device__ __forceinline__ void block_colsum_store(const float (&part)[K][N], const RowMap &rm, int C, float *out, int nb) {
    // (tpr * rpp == 256 for these: every thread is active)
    if (rm.tpr == 4) return block_colsum_store_g<N, K, 4>(part, C, out, nb);
    if (rm.tpr == 8) return block_colsum_store_g<N, K, 8>(part, C, out, nb);
    if (rm.tpr == 16) return block_colsum_store_g<N, K, 16>(part, C, out, nb);
    if (rm.tpr == 32) return block_colsum_store_g<N, K, 32>(part, C, out, nb);
    // general path (>= 64 threads per row: at most four row slots; odd channel counts): one quantity at a time through the same scratch
    float *const red = colsum_scratch();         // [256][N]
#pragma unroll
    for (int k = 0; k < K; ++k) {
        if (k) __syncthreads();
#pragma unroll
        for (int j = 0; j < N; ++j) red[threadIdx.x * N + j] = rm.active ? part[k][j] : 0.f;
        __syncthreads();
        if (threadIdx.x < rm.tpr) {
#pragma unroll
            for (int j = 0; j < N; ++j) {
                float s = 0.f;
                for (int r = 0; r < rm.rpp; ++r) s += red[(r * rm.tpr + threadIdx.x) * N + j];
                out[((long)k * nb + blockIdx.x) * C + threadIdx.x * N + j] = s;
            }
        }
    }
}

static inline int colsum_grid(long M, int C, int vec) {
    int tpr = C / vec, rpp = 256 / tpr;
    if (rpp < 1) rpp = 1;
    long g = (M + (long)rpp * 4 - 1) / ((long)rpp * 4);
    const int cap = 256;
    if (g > cap) g = cap;       // default 1 workgroup per CU (measured best: 64..1024 swept); keeps the finalisation short (workspace contract: <= 1024)
    if (g < 1) g = 1;
    return (int)g;
}

// FIN 0: (sum x, sum x^2) -> mean, biased var;  FIN 1: two sums -> two f32 outputs;  FIN 2: one sum -> o0
template <int FIN>
__global__ __launch_bounds__(256) void reduce_finalize_kernel(const float *__restrict__ part, int nb, int C, long M,
                                                              float *__restrict__ o0, float *__restrict__ o1, int nout,
                                                              float *__restrict__ mm = nullptr, float *__restrict__ mv = nullptr,
                                                              float omd = 0.f) {
    // 16 columns x 16 row groups per block: every thread sums nb/16 partials with 4 independent f64 chains
    // (the first version walked up to 1024 partials serially per thread: 77 us of pure latency per call)
    constexpr int K = FIN == 2 ? 1 : 2;
    __shared__ double red[K][16][17];
    const int col = threadIdx.x & 15, rg = threadIdx.x >> 4;
    const int c = blockIdx.x * 16 + col;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
        if (c < C) {
            const float *p = part + (long)k * nb * C + c;
            int b = rg;
            for (; b + 48 < nb; b += 64) {
                s0 += (double)p[(long)b * C];
                s1 += (double)p[(long)(b + 16) * C];
                s2 += (double)p[(long)(b + 32) * C];
                s3 += (double)p[(long)(b + 48) * C];
            }
            for (; b < nb; b += 16) s0 += (double)p[(long)b * C];
        }
        red[k][rg][col] = (s0 + s1) + (s2 + s3);
    }
    __syncthreads();
    if (rg == 0 && c < nout) {
        double t[K];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            double a = 0.0;
#pragma unroll
            for (int r = 0; r < 16; ++r) a += red[k][r][col];
            t[k] = a;
        }
        if (FIN == 0) {
            double dm = t[0] / (double)M;                       // mean of (x - shift)
            double var = t[K - 1] / (double)M - dm * dm;
            double mean = (double)part[(long)2 * nb * C + c] + dm;
            const float fm = (float)mean, fv = (float)(var > 0.0 ? var : 0.0);
            o0[c] = fm;
            o1[c] = fv;
            if (mm) {   // fused assign_moving_average (UPDATE_OPS)
                mm[c] = bn_ema(mm[c], fm, omd);
                mv[c] = bn_ema(mv[c], fv, omd);
            }
        } else if (FIN == 1) {
            o0[c] = (float)t[0];
            o1[c] = (float)t[K - 1];
        } else {
            o0[c] = (float)t[0];
        }
    }
}
