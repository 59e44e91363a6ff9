// Options of the YOLOv2 loss beyond the box term (head.hip: loss_kernel<T, MODE, CLS, EXT>; tests/loss_opt_ref.py is the
// specification): the ignore threshold of Darknet's region layer, the IoU objectness target (rescore) and a cross-entropy / focal class term
// with label smoothing.  All off is the loss as it was: the instantiations with CLS == Y2_CLS_MSE and EXT == false carry nothing of this file.
#pragma once

enum { Y2_CLS_MSE = 0, Y2_CLS_CE = 1, Y2_CLS_FOCAL = 2, Y2_CLS_MODES = 3 };

// what the kernel reads of yolo2_loss_options, by value
struct loss_opts {
    float ignore_thresh;     // 0: off
    int rescore;
    float label_smoothing;
    float focal_gamma;
};

// Ground truth boxes of one image staged per workgroup: absolute corners in grid units and the area label, structure of arrays.  An image
// with more object cells than this, or a workgroup that covers more than two images (tiny grids), reads the label rows through L1 / L2.
#define Y2_GT_CAP 512

__device__ __forceinline__ float gt_iou_(float px1, float py1, float px2, float py2, float area_p, float tx1, float ty1, float tx2, float ty2,
                                         float area_t) {
    const float ix = fmaxf(fminf(px2, tx2) - fmaxf(px1, tx1), 0.0f);
    const float iy = fmaxf(fminf(py2, ty2) - fmaxf(py1, ty1), 0.0f);
    const float inter = ix * iy;
    if (!(inter > 0.0f)) return 0.0f;       // (0 / positive union is 0 as well; this only spares the division)
    return inter / fmaxf((area_t + area_p) - inter, 1e-10f);
}

// the label rows of image b, every object cell: the path without staging
__device__ __forceinline__ float gt_scan_direct_(const float *__restrict__ mask, const float *__restrict__ off_min, const float *__restrict__ off_max,
                                                 const float *__restrict__ areas, long b, int cells, int cell_w, float px1, float py1, float px2,
                                                 float py2, float area_p) {
    float M = 0.0f;
    for (int j = 0; j < cells; ++j) {
        const long idx = b * cells + j;
        if (mask[idx] != 0.0f) {
            const float cx = (float)(j % cell_w), cy = (float)(j / cell_w);
            M = fmaxf(M, gt_iou_(px1, py1, px2, py2, area_p, cx + off_min[idx * 2], cy + off_min[idx * 2 + 1], cx + off_max[idx * 2],
                                 cy + off_max[idx * 2 + 1], areas[idx]));
        }
    }
    return M;
}

// M of the calling lane: the largest IoU of its predicted box (absolute corners, grid units) with a ground truth box of its image -- the object
// cells of the label tensors, one box per cell, the lane's own cell included; 0 where the image has none.  Called by every thread of the
// 256-thread workgroup (it synchronises); `act` false for idle lanes.  The object cells of an image are compacted into LDS in cell order
// with a ballot and a prefix over the four waves: no atomics, and a maximum does not depend on the order anyway.
__device__ __forceinline__ float gt_scan(const float *__restrict__ mask, const float *__restrict__ off_min, const float *__restrict__ off_max,
                                         const float *__restrict__ areas, int B, int cells, int cell_w, int LPC, bool act, long cell_id, float px1,
                                         float py1, float px2, float py2, float area_p) {
    __shared__ float gt[5][Y2_GT_CAP];
    __shared__ int wcnt[4];
    const long total = (long)B * cells;
    const long c_first = ((long)blockIdx.x * 256) / LPC;
    long c_last = ((long)blockIdx.x * 256 + 255) / LPC;
    if (c_last > total - 1) c_last = total - 1;
    const long b_first = c_first / cells, b_last = c_last / cells;       // workgroup-uniform
    const long b = act ? cell_id / cells : -1;
    if (b_last - b_first > 1)                                             // a tiny grid: up to 256 images here, a few cells each
        return act ? gt_scan_direct_(mask, off_min, off_max, areas, b, cells, cell_w, px1, py1, px2, py2, area_p) : 0.0f;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    float M = 0.0f;
    for (long bb = b_first; bb <= b_last; ++bb) {
        int n = 0;                                                        // object cells of image bb so far (uniform)
        for (int base = 0; base < cells; base += 256) {
            const int j = base + tid;
            const long idx = bb * cells + j;
            const bool obj = j < cells && mask[idx] != 0.0f;
            const unsigned long long bal = __ballot(obj);
            if (lane == 0) wcnt[wave] = __popcll(bal);
            __syncthreads();
            int slot = n + __popcll(bal & ((1ull << lane) - 1ull));
            for (int w = 0; w < wave; ++w) slot += wcnt[w];
            n += wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
            if (obj && slot < Y2_GT_CAP) {
                const float cx = (float)(j % cell_w), cy = (float)(j / cell_w);
                gt[0][slot] = cx + off_min[idx * 2];
                gt[1][slot] = cy + off_min[idx * 2 + 1];
                gt[2][slot] = cx + off_max[idx * 2];
                gt[3][slot] = cy + off_max[idx * 2 + 1];
                gt[4][slot] = areas[idx];
            }
            __syncthreads();                                              // the list is visible; wcnt may be rewritten
        }
        if (b == bb) {
            if (n <= Y2_GT_CAP) {
                for (int k = 0; k < n; ++k) M = fmaxf(M, gt_iou_(px1, py1, px2, py2, area_p, gt[0][k], gt[1][k], gt[2][k], gt[3][k], gt[4][k]));
            } else {
                M = gt_scan_direct_(mask, off_min, off_max, areas, b, cells, cell_w, px1, py1, px2, py2, area_p);
            }
        }
        __syncthreads();                                                  // before the next image overwrites the list
    }
    return M;
}

// (1 - p)^(gamma - 1) for gamma >= 1; the usual exponents 1 and 2 (a uniform branch) do without powf, which was four fifths of what the focal term added to the launch (profiles/loss_options.md)
__device__ __forceinline__ float focal_pow_(float om, float gamma) {
    if (gamma == 2.0f) return om;
    if (gamma == 1.0f) return 1.0f;
    return powf(om, gamma - 1.0f);
}

// Class term of one responsible lane, cross-entropy (FOCAL false) or focal, on the smoothed target tt_k = (1 - eps) t_k + eps T / C, T = sum t_k
// (the label row may be multi-hot).  Returns -sum_k tt_k (1 - p_k)^gamma log p_k; with dp != nullptr writes scale * d/dz_j into dp[j]:
//     A_k = tt_k [gamma (1 - p_k)^(gamma - 1) p_k log p_k - (1 - p_k)^gamma]   ( = dL/dp_k * p_k, no 1 / p ),   dz_j = A_j - p_j sum_k A_k
// log p_k is the log-softmax (z_k - max) - log sum exp, never log(p); the sum is held as 1 + (the terms other than the first maximum), so that
// log sum exp = log1p(rest) and 1 - p_max = rest / sum keep their relative accuracy where the softmax saturates.  gamma >= 1 here (gamma == 0 is
// launched as cross-entropy).
template <bool FOCAL, typename T>
__device__ __forceinline__ float class_term(const T *__restrict__ zp, const float *__restrict__ tp, int C, float eps, float gamma, float scale,
                                            T *__restrict__ dp) {
    float mx = -INFINITY;
    int kmax = 0;
    for (int k = 0; k < C; ++k) {
        const float v = (float)zp[k];
        if (v > mx) { mx = v; kmax = k; }
    }
    float rest = 0.f, Tsum = 0.f;
    for (int k = 0; k < C; ++k) {
        if (k != kmax) rest += expf((float)zp[k] - mx);
        Tsum += tp[k];
    }
    const float den = 1.0f + rest, lse = log1pf(rest);
    const float sm = eps * Tsum / (float)C, keep = 1.0f - eps;
    float obj = 0.f, S = 0.f;
    for (int k = 0; k < C; ++k) {
        const float tt = keep * tp[k] + sm;
        const float d = (float)zp[k] - mx;
        const float logp = (k == kmax ? 0.0f : d) - lse;
        if constexpr (FOCAL) {
            const float p = (k == kmax ? 1.0f : expf(d)) / den;
            const float om = k == kmax ? rest / den : 1.0f - p;
            const float pw1 = focal_pow_(om, gamma), pw = pw1 * om;
            obj -= tt * (pw * logp);
            S += tt * (gamma * pw1 * (p * logp) - pw);
        } else {
            obj -= tt * logp;
            S -= tt;
        }
    }
    if (dp) {
        for (int k = 0; k < C; ++k) {
            const float tt = keep * tp[k] + sm;
            const float d = (float)zp[k] - mx;
            const float p = (k == kmax ? 1.0f : expf(d)) / den;
            float Ak = -tt;
            if constexpr (FOCAL) {
                const float logp = (k == kmax ? 0.0f : d) - lse;
                const float om = k == kmax ? rest / den : 1.0f - p;
                const float pw1 = focal_pow_(om, gamma);
                Ak = tt * (gamma * pw1 * (p * logp) - pw1 * om);
            }
            dp[k] = (T)(scale * (Ak - p * S));
        }
    }
    return obj;
}
