// Objectness-scaled distillation of one YOLOv2 head into another on gfx950 (Mehta & Ozturk, "Object detection at 200 frames per second",
// ECCV-W 2018; tests/distill_ref.py is the specification): the student's objectness, box and class outputs are pulled
// towards a frozen teacher's, the box and class terms weighted by the teacher's objectness.  The teacher is a constant: no derivative
// flows through it.
//
// The lane mapping and the sums are loss_kernel's (head.hip): one lane per (image, cell, anchor), the anchors of a cell in one power-of-two
// lane group, the class softmax serial in the lane; three partial sums per workgroup stored into the caller's workspace, reduced in index
// order by a second tiny launch.  No atomics: the result is bitwise reproducible.  The gradient is ADDED into dlogits, which the loss
// launch has written: dl = store(f32(dl) + g) over the real channels, padding channels untouched.  Built with FP contraction off, so that
// g is rounded before the addition (a start at zero plus a second start at d0 differ by exactly one f32 addition).
#include "common.h"
#pragma clang fp contract(off)
#include "head_math.h"
#include "box_loss.h"      // dsigmoidf_

enum { Y2_DISTILL_MSE = 0, Y2_DISTILL_KL = 1, Y2_DISTILL_TERMS = 2 };

// what the kernel reads of yolo2_distill_options, by value: the three weights already multiplied by the global one
struct distill_opts {
    int scale;          // 1: box and class terms weighted by sigmoid(teacher objectness)
    float T, inv_T;
    float g_obj, g_coords, g_prob;
};

// max and sum of expf((z - max) / T) of C class logits
template <typename T>
__device__ __forceinline__ void softmax_stats_(const T *__restrict__ z, int C, float inv_T, float &mx, float &den) {
    mx = -INFINITY;
    for (int k = 0; k < C; ++k) mx = fmaxf(mx, (float)z[k]);
    den = 0.f;
    for (int k = 0; k < C; ++k) den += expf(((float)z[k] - mx) * inv_T);
}

template <typename TS, typename TT, int CLS>
__global__ __launch_bounds__(256) void distill_kernel(const TS *__restrict__ student, int ld_s, const TT *__restrict__ teacher, int ld_t,
                                                      TS *__restrict__ dlogits, float *__restrict__ partial, int B, int cells, int A, int C,
                                                      int LPC, distill_opts o) {
    const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long cell_id = gid / LPC;  // flat (b, cell)
    const int a = (int)(gid % LPC);
    const bool act = cell_id < (long)B * cells && a < A;
    const float cnt = (float)((long)B * cells * A);
    const int D = 5 + C;

    float s0 = 0.f, s1 = 0.f, s2 = 0.f;      // objectness, coords, prob partial sums
    if (act) {
        const TS *sp = student + cell_id * ld_s + a * D;
        const TT *tp = teacher + cell_id * ld_t + a * D;
        float zs[5], zt[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) { zs[k] = (float)sp[k]; zt[k] = (float)tp[k]; }
        const float to = sigmoidf_(zt[0]);
        const float m = o.scale ? to : 1.0f;
        const float d0 = sigmoidf_(zs[0]) - to;
        const float dx = sigmoidf_(zs[1]) - sigmoidf_(zt[1]), dy = sigmoidf_(zs[2]) - sigmoidf_(zt[2]);
        const float dw = zs[3] - zt[3], dh = zs[4] - zt[4];      // anchors are shared: the log ratio of the two boxes' sides, no exp
        s0 = d0 * d0;
        s1 = m * (dx * dx + dy * dy + dw * dw + dh * dh);
        // class term on p = softmax(s / T), q = softmax(t / T)
        float mxs, dens, mxt, dent;
        softmax_stats_(sp + 5, C, o.inv_T, mxs, dens);
        softmax_stats_(tp + 5, C, o.inv_T, mxt, dent);
        float term = 0.f, dot = 0.f;
        if constexpr (CLS == Y2_DISTILL_MSE) {
            for (int k = 0; k < C; ++k) {
                const float p = expf(((float)sp[5 + k] - mxs) * o.inv_T) / dens;
                const float q = expf(((float)tp[5 + k] - mxt) * o.inv_T) / dent;
                const float e = p - q;
                term += e * e;
                dot += e * p;
            }
            s2 = m * term;
        } else {
            // T^2 sum_k q_k (log q_k - log p_k), the logarithms from the log-softmax
            const float lses = logf(dens), lset = logf(dent);
            for (int k = 0; k < C; ++k) {
                const float lp = ((float)sp[5 + k] - mxs) * o.inv_T - lses;
                const float lq = ((float)tp[5 + k] - mxt) * o.inv_T - lset;
                const float q = expf(((float)tp[5 + k] - mxt) * o.inv_T) / dent;
                term += q * (lq - lp);
            }
            s2 = m * (o.T * o.T) * term;
        }
        if (dlogits) {
            TS *dp = dlogits + cell_id * ld_s + a * D;
            float g[5];
            g[0] = 2.0f * d0 * o.g_obj / cnt * dsigmoidf_(zs[0]);
            g[1] = 2.0f * m * dx * o.g_coords / cnt * dsigmoidf_(zs[1]);
            g[2] = 2.0f * m * dy * o.g_coords / cnt * dsigmoidf_(zs[2]);
            g[3] = 2.0f * m * dw * o.g_coords / cnt;
            g[4] = 2.0f * m * dh * o.g_coords / cnt;
#pragma unroll
            for (int k = 0; k < 5; ++k) dp[k] = (TS)((float)dp[k] + g[k]);
            if constexpr (CLS == Y2_DISTILL_MSE) {
                // d/ds_j sum_k (p_k - q_k)^2 = (2 / T) p_j (e_j - sum_k e_k p_k)
                const float gp = 2.0f * m * o.g_prob * o.inv_T / cnt;
                for (int k = 0; k < C; ++k) {
                    const float p = expf(((float)sp[5 + k] - mxs) * o.inv_T) / dens;
                    const float q = expf(((float)tp[5 + k] - mxt) * o.inv_T) / dent;
                    const float gk = gp * (p * ((p - q) - dot));
                    dp[5 + k] = (TS)((float)dp[5 + k] + gk);
                }
            } else {
                // d/ds_j T^2 KL(q || p) = T (p_j - q_j)
                const float gp = m * o.g_prob * o.T / cnt;
                for (int k = 0; k < C; ++k) {
                    const float p = expf(((float)sp[5 + k] - mxs) * o.inv_T) / dens;
                    const float q = expf(((float)tp[5 + k] - mxt) * o.inv_T) / dent;
                    const float gk = gp * (p - q);
                    dp[5 + k] = (TS)((float)dp[5 + k] + gk);
                }
            }
        }
    }
    // block reduction of the three sums
    s0 = wave_sum(s0); s1 = wave_sum(s1); s2 = wave_sum(s2);
    __shared__ float red[4][3];
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { red[wave][0] = s0; red[wave][1] = s1; red[wave][2] = s2; }
    __syncthreads();
    if (threadIdx.x < 3) {
        float t = 0.f;
        for (int w = 0; w < (int)(blockDim.x >> 6); ++w) t += red[w][threadIdx.x];
        partial[(long)blockIdx.x * 3 + threadIdx.x] = t;
    }
}

__global__ void distill_finalize_kernel(const float *__restrict__ partial, int nblocks, float cnt, float *__restrict__ objectives) {
    const int k = threadIdx.x >> 6, lane = threadIdx.x & 63;  // 3 waves, one objective each
    double acc = 0.0;
    for (int i = lane; i < nblocks; i += 64) acc += (double)partial[(long)i * 3 + k];
    acc = wave_sum_d(acc);
    if (lane == 0) objectives[k] = (float)(acc / (double)cnt);
}

static int distill_lanes_per_cell(int A) {
    int l = 1;
    while (l < A) l <<= 1;
    return l;
}

// bytes of the caller-owned scratch `ws` of the distill entries: three partials per 256-lane workgroup
extern "C" size_t yolo2_distill_workspace_bytes(int B, int cells, int A) {
    return (size_t)(3 * (((long)B * cells * distill_lanes_per_cell(A) + 255) / 256)) * sizeof(float);
}

extern "C" int yolo2_distill_partials(const void *student, int ld_s, int dtype_s, const void *teacher, int ld_t, int dtype_t, void *dlogits,
                                      float *ws, int B, int cell_h, int cell_w, int A, int C, void *stream, const yolo2_distill_options *opt) {
    Y2_CHECK_ARG(student && teacher && ws);
    Y2_CHECK_ARG(opt && opt->size == (int)sizeof(yolo2_distill_options));
    Y2_CHECK_ARG((dtype_s == YOLO2_F32 || dtype_s == YOLO2_BF16) && (dtype_t == YOLO2_F32 || dtype_t == YOLO2_BF16));
    Y2_CHECK_ARG(opt->class_term >= 0 && opt->class_term < Y2_DISTILL_TERMS && (opt->scale_by_objectness == 0 || opt->scale_by_objectness == 1));
    Y2_CHECK_ARG(opt->temperature > 0.0f && std::isfinite(opt->temperature));                                       // (a NaN fails the first)
    Y2_CHECK_ARG(opt->weight >= 0.0f && opt->w_objectness >= 0.0f && opt->w_coords >= 0.0f && opt->w_prob >= 0.0f);
    Y2_CHECK_ARG(std::isfinite(opt->weight) && std::isfinite(opt->w_objectness) && std::isfinite(opt->w_coords) && std::isfinite(opt->w_prob));
    Y2_CHECK_ARG(B > 0 && cell_h > 0 && cell_w > 0 && A > 0 && A <= 64 && C > 0 && ld_s >= A * (5 + C) && ld_t >= A * (5 + C));
    hipStream_t st = (hipStream_t)stream;
    const int LPC = distill_lanes_per_cell(A);
    const int cells = cell_h * cell_w;
    const int nblocks = cdiv((long)B * cells * LPC, 256);
    const distill_opts ko = {opt->scale_by_objectness, opt->temperature, 1.0f / opt->temperature, opt->weight * opt->w_objectness,
                             opt->weight * opt->w_coords, opt->weight * opt->w_prob};
#define Y2_DISTILL_LAUNCH(TS, TT, CLS) \
    distill_kernel<TS, TT, CLS><<<nblocks, 256, 0, st>>>((const TS *)student, ld_s, (const TT *)teacher, ld_t, (TS *)dlogits, ws, B, cells, A, C, LPC, ko)
#define Y2_DISTILL_LAUNCH2(CLS)                                                        \
    do {                                                                               \
        if (dtype_s == YOLO2_F32 && dtype_t == YOLO2_F32) Y2_DISTILL_LAUNCH(float, float, CLS); \
        else if (dtype_s == YOLO2_F32) Y2_DISTILL_LAUNCH(float, bf16, CLS);            \
        else if (dtype_t == YOLO2_F32) Y2_DISTILL_LAUNCH(bf16, float, CLS);            \
        else Y2_DISTILL_LAUNCH(bf16, bf16, CLS);                                       \
    } while (0)
    if (opt->class_term == Y2_DISTILL_MSE) Y2_DISTILL_LAUNCH2(Y2_DISTILL_MSE);
    else Y2_DISTILL_LAUNCH2(Y2_DISTILL_KL);
#undef Y2_DISTILL_LAUNCH2
#undef Y2_DISTILL_LAUNCH
    Y2_CHECK_LAUNCH();
    return YOLO2_OK;
}

extern "C" int yolo2_distill_objectives(const float *ws, float *objectives, int B, int cell_h, int cell_w, int A, void *stream) {
    Y2_CHECK_ARG(ws && objectives && B > 0 && cell_h > 0 && cell_w > 0 && A > 0 && A <= 64);
    const int nblocks = cdiv((long)B * cell_h * cell_w * distill_lanes_per_cell(A), 256);
    distill_finalize_kernel<<<1, 192, 0, (hipStream_t)stream>>>(ws, nblocks, (float)((long)B * cell_h * cell_w * A), objectives);
    Y2_CHECK_LAUNCH();
    return YOLO2_OK;
}
