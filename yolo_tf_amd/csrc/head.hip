// YOLOv2 head on gfx950: decode (detect) and the per-grid-cell anchor loss, forward + backward
// fused.  Replaces Model.__init__ / Objectives.__init__ (reference model/yolo2/__init__.py:28-94)
// and the tf.gradients of the weighted objectives (Builder.create_objectives :114-119).
//
// One lane per (image, cell, anchor); the anchors of a cell sit in one power-of-two lane group so
// the responsible-anchor selection (reduce_max over A, then exact float equality, :80-81) is a
// wavefront butterfly shuffle -- no LDS, no atomics.  The IoU is computed in the reference's
// operation order with FP contraction off, because `iou == max_A iou` is an exact compare.
// The four objective sums are reduced wave -> block -> a deterministic second pass.
#include "common.h"
#pragma clang fp contract(off)
#include "head_math.h"
#include "box_loss.h"
#include "loss_opts.h"

// MODE (box_loss.h): Y2_BOX_MSE regresses the responsible anchor's box with the reference's squared error on (sx, sy, sqrt w, sqrt h); the
// other modes put 1 - q of an IoU-family score in the `coords` slot and its closed-form gradient in channels 1..4, on the responsible lanes
// only.  A compile-time parameter: the mse instantiation carries none of the new arithmetic, atan2f exists only in the CIoU one.
// CLS and EXT (loss_opts.h): the class term (Y2_CLS_MSE: the reference's squared error on the softmax) and whether the launch carries the ignore
// threshold / the IoU objectness target, both read from `opt` behind workgroup-uniform branches.  <T, MODE, Y2_CLS_MSE, false> is the kernel as
// it was before these options existed.
template <typename T, int MODE, int CLS, bool EXT>
__global__ __launch_bounds__(256) void loss_kernel(
    const T *__restrict__ logits, int ld, const float *__restrict__ anchors, const float *__restrict__ mask,
    const float *__restrict__ prob, const float *__restrict__ coords, const float *__restrict__ off_min,
    const float *__restrict__ off_max, const float *__restrict__ areas, float w_best, float w_normal,
    float w_coords, float w_prob, T *__restrict__ dlogits, float *__restrict__ partial, int B, int cell_h,
    int cell_w, int A, int C, int LPC, loss_opts opt) {
    const int cells = cell_h * cell_w;
    const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long cell_id = gid / LPC;  // flat (b, cell)
    const int a = (int)(gid % LPC);
    const bool act = cell_id < (long)B * cells && a < A;
    const float cnt = (float)((long)B * cells * A);
    const int D = 5 + C;

    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;  // iou_best, iou_normal, coords, prob partial sums
    float iou = -INFINITY;
    float z[5], sg[3], wh[2], sq[2], tc[4], m = 0.f;      // (sq, tc -- sqrt of the predicted size in grid units, the `coords` label -- are the mse mode's alone)
    const T *lp = nullptr;
    float gx1 = 0.f, gy1 = 0.f, gx2 = 0.f, gy2 = 0.f, garea = 0.f;      // EXT: the predicted box in grid units (cell_xy + offset_xy_min / max) and its area
    if (act) {
        lp = logits + cell_id * ld + a * D;
#pragma unroll
        for (int k = 0; k < 5; ++k) z[k] = (float)lp[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) sg[k] = sigmoidf_(z[k]);
        wh[0] = expf(z[3]) * anchors[2 * a + 0];
        wh[1] = expf(z[4]) * anchors[2 * a + 1];
        const float area_p = wh[0] * wh[1];
        const float hx = wh[0] / 2.0f, hy = wh[1] / 2.0f;
        const float pminx = sg[1] - hx, pminy = sg[2] - hy, pmaxx = sg[1] + hx, pmaxy = sg[2] + hy;
        if constexpr (EXT) {
            const int cell = (int)(cell_id % cells);
            const float cx = (float)(cell % cell_w), cy = (float)(cell / cell_w);
            gx1 = cx + pminx, gy1 = cy + pminy, gx2 = cx + pmaxx, gy2 = cy + pmaxy, garea = area_p;
        }
        if constexpr (MODE == Y2_BOX_MSE) {
            sq[0] = sqrtf(wh[0] / (float)cell_w);
            sq[1] = sqrtf(wh[1] / (float)cell_h);
        }
        m = mask[cell_id];
        const float tminx = off_min[cell_id * 2], tminy = off_min[cell_id * 2 + 1];
        const float tmaxx = off_max[cell_id * 2], tmaxy = off_max[cell_id * 2 + 1];
        const float ix = fmaxf(fminf(pmaxx, tmaxx) - fmaxf(pminx, tminx), 0.0f);
        const float iy = fmaxf(fminf(pmaxy, tmaxy) - fmaxf(pminy, tminy), 0.0f);
        const float inter = ix * iy;
        const float uni = fmaxf((areas[cell_id] + area_p) - inter, 1e-10f);
        iou = inter / uni;
        if constexpr (MODE == Y2_BOX_MSE) {
#pragma unroll
            for (int k = 0; k < 4; ++k) tc[k] = coords[cell_id * 4 + k];
        }
    }
    // best anchor of the cell: butterfly max inside the LPC-lane group
    float best = iou;
    for (int o = LPC >> 1; o > 0; o >>= 1) best = fmaxf(best, __shfl_xor(best, o, 64));
    // ignore threshold: M = the largest IoU of the lane's box with a ground truth box of its image (every thread takes part in the staging)
    float M = 0.f;
    if constexpr (EXT) {
        if (opt.ignore_thresh > 0.0f) M = gt_scan(mask, off_min, off_max, areas, B, cells, cell_w, LPC, act, cell_id, gx1, gy1, gx2, gy2, garea);
    }

    if (act) {
        const float mb = m * (iou == best ? 1.0f : 0.0f);
        float tgt = mb;                  // the objectness target: 1 on the responsible lanes (their own matching IoU with rescore), 0 elsewhere
        bool ignored = false;            // not responsible and M > ignore_thresh: no part in iou_normal, no objectness gradient
        if constexpr (EXT) {
            if (opt.rescore && mb != 0.0f) tgt = iou;
            ignored = opt.ignore_thresh > 0.0f && mb == 0.0f && M > opt.ignore_thresh;
        }
        const float d_iou = sg[0] - tgt;
        const float iou_dist = d_iou * d_iou;
        s0 = mb * iou_dist;
        s1 = ignored ? 0.0f : (1.0f - mb) * iou_dist;
        float dc0 = 0.f, dc1 = 0.f, dc2 = 0.f, dc3 = 0.f;      // mse: prediction - label of (sx, sy, sqrt w, sqrt h)
        float gbox[4] = {0.f, 0.f, 0.f, 0.f};                  // the other modes: dq / d(sx, sy, w, h) of a responsible lane
        if constexpr (MODE == Y2_BOX_MSE) {
            dc0 = sg[1] - tc[0], dc1 = sg[2] - tc[1], dc2 = sq[0] - tc[2], dc3 = sq[1] - tc[3];
            s2 = mb * (dc0 * dc0) + mb * (dc1 * dc1) + mb * (dc2 * dc2) + mb * (dc3 * dc3);
        } else if (mb != 0.0f) {
            const float q = box_score<MODE>(sg[1], sg[2], wh[0], wh[1], off_min[cell_id * 2], off_min[cell_id * 2 + 1], off_max[cell_id * 2],
                                            off_max[cell_id * 2 + 1], areas[cell_id], gbox);
            s2 = mb * (1.0f - q);
        }
        // softmax over classes (two passes over the logits; they are L1-resident).  Only the responsible anchors need it: the class term
        // and its gradient carry the factor mask_best (model/yolo2/__init__.py:87,94), which is 0 for every other lane -- a handful of
        // lanes per image instead of all 845 (with 80 classes the three class loops were 2/3 of this kernel: 45 -> 15 us at batch 8).
        const bool resp = mb != 0.0f;
        float mx = -INFINITY, den = 1.f;
        const float *tp = prob + cell_id * C;
        float sp = 0.f, dot = 0.f;
        const float gp = 2.0f * mb * w_prob / cnt;
        if constexpr (CLS != Y2_CLS_MSE) {
            // cross-entropy / focal (loss_opts.h): objective and gradient of a responsible lane in one call, the other lanes' class channels zeroed
            T *dcls = dlogits ? dlogits + cell_id * ld + a * D + 5 : nullptr;
            if (resp) sp = class_term<CLS == Y2_CLS_FOCAL, T>(lp + 5, tp, C, opt.label_smoothing, opt.focal_gamma, mb * w_prob / cnt, dcls);
            else if (dcls) for (int k = 0; k < C; ++k) dcls[k] = (T)0.f;
        } else if (resp) {
            for (int k = 0; k < C; ++k) mx = fmaxf(mx, (float)lp[5 + k]);
            den = 0.f;
            for (int k = 0; k < C; ++k) den += expf((float)lp[5 + k] - mx);
            for (int k = 0; k < C; ++k) {
                float p = expf((float)lp[5 + k] - mx) / den;
                float e = p - tp[k];
                sp += e * e;
                dot += (gp * e) * p;
            }
        }
        s3 = mb * sp;
        if (dlogits) {
            T *dp = dlogits + cell_id * ld + a * D;
            const float w_obj = w_best * mb + w_normal * (1.0f - mb);
            dp[0] = ignored ? (T)0.f : (T)(2.0f * (sg[0] - tgt) * w_obj / cnt * sg[0] * (1.0f - sg[0]));
            if constexpr (MODE == Y2_BOX_MSE) {
                dp[1] = (T)(2.0f * mb * dc0 * w_coords / cnt * sg[1] * (1.0f - sg[1]));
                dp[2] = (T)(2.0f * mb * dc1 * w_coords / cnt * sg[2] * (1.0f - sg[2]));
                dp[3] = (T)(2.0f * mb * dc2 * w_coords / cnt * sq[0] / 2.0f);
                dp[4] = (T)(2.0f * mb * dc3 * w_coords / cnt * sq[1] / 2.0f);
            } else if (resp) {
                // d(w_coords * mb * (1 - q) / cnt) through sx = sigmoid(z1), sy = sigmoid(z2), w = exp(z3) * aw, h = exp(z4) * ah
                const float gc = -(mb * w_coords / cnt);
                dp[1] = (T)(gc * gbox[0] * dsigmoidf_(z[1]));
                dp[2] = (T)(gc * gbox[1] * dsigmoidf_(z[2]));
                dp[3] = (T)(gc * gbox[2] * wh[0]);
                dp[4] = (T)(gc * gbox[3] * wh[1]);
            } else {
                for (int k = 1; k < 5; ++k) dp[k] = (T)0.f;
            }
            if constexpr (CLS == Y2_CLS_MSE) {
                if (resp) {
                    for (int k = 0; k < C; ++k) {
                        float p = expf((float)lp[5 + k] - mx) / den;
                        float d = gp * (p - tp[k]);
                        dp[5 + k] = (T)(p * (d - dot));
                    }
                } else {
                    for (int k = 0; k < C; ++k) dp[5 + k] = (T)0.f;
                }
            }
            if (a == 0)
                for (int k = A * D; k < ld; ++k) dlogits[cell_id * ld + k] = (T)0.f;
        }
    }
    // block reduction of the four sums
    s0 = wave_sum(s0); s1 = wave_sum(s1); s2 = wave_sum(s2); s3 = wave_sum(s3);
    __shared__ float red[4][4];
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { red[wave][0] = s0; red[wave][1] = s1; red[wave][2] = s2; red[wave][3] = s3; }
    __syncthreads();
    if (threadIdx.x < 4) {
        float t = 0.f;
        for (int w = 0; w < (int)(blockDim.x >> 6); ++w) t += red[w][threadIdx.x];
        partial[(long)blockIdx.x * 4 + threadIdx.x] = t;
    }
}

__global__ void loss_finalize_kernel(const float *__restrict__ partial, int nblocks, float cnt, float *__restrict__ objectives) {
    const int k = threadIdx.x >> 6, lane = threadIdx.x & 63;  // 4 waves, one objective each
    double acc = 0.0;
    for (int i = lane; i < nblocks; i += 64) acc += (double)partial[(long)i * 4 + k];
    acc = wave_sum_d(acc);
    if (lane == 0) objectives[k] = (float)(acc / (double)cnt);
}

static int lanes_per_cell(int A) {
    int l = 1;
    while (l < A) l <<= 1;
    return l;
}

static yolo2_loss_options default_loss_options(int box_loss = Y2_BOX_MSE) {
    yolo2_loss_options o = {(int)sizeof(yolo2_loss_options), box_loss, Y2_CLS_MSE, 0, 0.0f, 0.0f, 2.0f};
    return o;
}

static int loss_impl(const void *logits, int ld, const float *anchors, const float *mask, const float *prob,
                     const float *coords, const float *off_min, const float *off_max, const float *areas,
                     const float *hparam, float *objectives, void *dlogits, float *ws, int B, int cell_h,
                     int cell_w, int A, int C, int dtype, void *stream, const yolo2_loss_options &o = default_loss_options()) {
    Y2_CHECK_ARG(logits && anchors && mask && prob && coords && off_min && off_max && areas && hparam && ws);
    const int box_loss = o.box_loss;
    Y2_CHECK_ARG(box_loss >= 0 && box_loss < Y2_BOX_MODES);
    Y2_CHECK_ARG(o.class_loss >= 0 && o.class_loss < Y2_CLS_MODES && (o.rescore == 0 || o.rescore == 1));
    Y2_CHECK_ARG(o.ignore_thresh == 0.0f || (o.ignore_thresh > 0.0f && o.ignore_thresh < 1.0f));                 // (a NaN fails both)
    Y2_CHECK_ARG(o.label_smoothing >= 0.0f && o.label_smoothing < 1.0f && (o.class_loss != Y2_CLS_MSE || o.label_smoothing == 0.0f));
    Y2_CHECK_ARG(o.class_loss != Y2_CLS_FOCAL || o.focal_gamma == 0.0f || (o.focal_gamma >= 1.0f && std::isfinite(o.focal_gamma)));
    Y2_CHECK_ARG(B > 0 && cell_h > 0 && cell_w > 0 && A > 0 && A <= 64 && C > 0 && ld >= A * (5 + C));
    hipStream_t st = (hipStream_t)stream;
    const int LPC = lanes_per_cell(A);
    const long threads = (long)B * cell_h * cell_w * LPC;
    const int nblocks = cdiv(threads, 256);
    float hp[4];
    // hparam is a host pointer: 4 weights {iou_best, iou_normal, coords, prob}
    hp[0] = hparam[0]; hp[1] = hparam[1]; hp[2] = hparam[2]; hp[3] = hparam[3];
    // focal with gamma 0 is the cross-entropy; EXT only where the ignore threshold or the IoU target is on: all off is the launch as it was
    const int cls = o.class_loss == Y2_CLS_FOCAL && o.focal_gamma == 0.0f ? Y2_CLS_CE : o.class_loss;
    const bool ext = o.ignore_thresh > 0.0f || o.rescore != 0;
    const loss_opts ko = {o.ignore_thresh, o.rescore, o.label_smoothing, o.focal_gamma};
#define Y2_LOSS_LAUNCH4(MODE, CLS, EXT)                                                                                                                    \
    Y2_DISPATCH_DTYPE(dtype, (loss_kernel<T, MODE, CLS, EXT><<<nblocks, 256, 0, st>>>((const T *)logits, ld, anchors, mask, prob, coords, off_min, off_max, \
                                                                                      areas, hp[0], hp[1], hp[2], hp[3], (T *)dlogits, ws, B, cell_h,     \
                                                                                      cell_w, A, C, LPC, ko)))
#define Y2_LOSS_LAUNCH3(MODE, CLS)                 \
    do {                                           \
        if (ext) Y2_LOSS_LAUNCH4(MODE, CLS, true); \
        else Y2_LOSS_LAUNCH4(MODE, CLS, false);    \
    } while (0)
#define Y2_LOSS_LAUNCH(MODE)                                           \
    do {                                                               \
        if (cls == Y2_CLS_MSE) Y2_LOSS_LAUNCH3(MODE, Y2_CLS_MSE);      \
        else if (cls == Y2_CLS_CE) Y2_LOSS_LAUNCH3(MODE, Y2_CLS_CE);   \
        else Y2_LOSS_LAUNCH3(MODE, Y2_CLS_FOCAL);                      \
    } while (0)
    switch (box_loss) {
        case Y2_BOX_MSE: Y2_LOSS_LAUNCH(Y2_BOX_MSE); break;
        case Y2_BOX_IOU: Y2_LOSS_LAUNCH(Y2_BOX_IOU); break;
        case Y2_BOX_GIOU: Y2_LOSS_LAUNCH(Y2_BOX_GIOU); break;
        case Y2_BOX_DIOU: Y2_LOSS_LAUNCH(Y2_BOX_DIOU); break;
        default: Y2_LOSS_LAUNCH(Y2_BOX_CIOU); break;
    }
#undef Y2_LOSS_LAUNCH
#undef Y2_LOSS_LAUNCH3
#undef Y2_LOSS_LAUNCH4
    if (objectives) loss_finalize_kernel<<<1, 256, 0, st>>>(ws, nblocks, (float)((long)B * cell_h * cell_w * A), objectives);
    Y2_CHECK_LAUNCH();
    return YOLO2_OK;
}
// bytes of the caller-owned scratch `ws` of the loss entries: four partials per 256-lane workgroup + the four sums
extern "C" size_t yolo2_loss_workspace_bytes(int B, int cells, int A) {
    int lpc = 1;
    while (lpc < A) lpc *= 2;
    return (size_t)(4 * (((long)B * cells * lpc + 255) / 256) + 4) * sizeof(float);
}
extern "C" int yolo2_loss(const void *logits, int ld, const float *anchors, const float *mask, const float *prob,
                          const float *coords, const float *off_min, const float *off_max, const float *areas,
                          const float *hparam, float *objectives, void *dlogits, float *ws, int B, int cell_h,
                          int cell_w, int A, int C, int dtype, void *stream) {
    Y2_CHECK_ARG(objectives);
    return loss_impl(logits, ld, anchors, mask, prob, coords, off_min, off_max, areas, hparam, objectives, dlogits, ws, B, cell_h, cell_w, A, C, dtype, stream);
}
// The training step needs only dlogits; the four objective values are read a few times a minute (summaries).  yolo2_loss_partials runs the
// loss kernel alone (per-workgroup partial sums stay in ws), yolo2_loss_objectives reduces them when somebody asks -- one launch less
// on the step's critical path.  Together they equal yolo2_loss.
extern "C" int yolo2_loss_partials(const void *logits, int ld, const float *anchors, const float *mask, const float *prob,
                                   const float *coords, const float *off_min, const float *off_max, const float *areas,
                                   const float *hparam, void *dlogits, float *ws, int B, int cell_h, int cell_w, int A, int C, int dtype, void *stream) {
    return loss_impl(logits, ld, anchors, mask, prob, coords, off_min, off_max, areas, hparam, nullptr, dlogits, ws, B, cell_h, cell_w, A, C, dtype, stream);
}
// The same two entries with the box regression loss chosen (box_loss.h: 0 = mse, today's loss, bit for bit; 1 = iou, 2 = giou, 3 = diou, 4 = ciou).
// Workspace and yolo2_loss_objectives serve every mode.
extern "C" int yolo2_loss_box(const void *logits, int ld, const float *anchors, const float *mask, const float *prob,
                              const float *coords, const float *off_min, const float *off_max, const float *areas,
                              const float *hparam, float *objectives, void *dlogits, float *ws, int B, int cell_h,
                              int cell_w, int A, int C, int dtype, void *stream, int box_loss) {
    Y2_CHECK_ARG(objectives);
    return loss_impl(logits, ld, anchors, mask, prob, coords, off_min, off_max, areas, hparam, objectives, dlogits, ws, B, cell_h, cell_w, A, C, dtype, stream, default_loss_options(box_loss));
}
extern "C" int yolo2_loss_box_partials(const void *logits, int ld, const float *anchors, const float *mask, const float *prob,
                                       const float *coords, const float *off_min, const float *off_max, const float *areas,
                                       const float *hparam, void *dlogits, float *ws, int B, int cell_h, int cell_w, int A, int C, int dtype,
                                       void *stream, int box_loss) {
    return loss_impl(logits, ld, anchors, mask, prob, coords, off_min, off_max, areas, hparam, nullptr, dlogits, ws, B, cell_h, cell_w, A, C, dtype, stream, default_loss_options(box_loss));
}
// One options struct for every loss option (include/yolo2_hip.h: yolo2_loss_options; loss_opts.h); with the defaults these are yolo2_loss /
// yolo2_loss_partials, with only box_loss set yolo2_loss_box / yolo2_loss_box_partials, bit for bit.  A NULL or differently sized struct and
// every out-of-range field are argument errors: nothing is launched.
extern "C" int yolo2_loss_ex(const void *logits, int ld, const float *anchors, const float *mask, const float *prob,
                             const float *coords, const float *off_min, const float *off_max, const float *areas,
                             const float *hparam, float *objectives, void *dlogits, float *ws, int B, int cell_h,
                             int cell_w, int A, int C, int dtype, void *stream, const yolo2_loss_options *opt) {
    Y2_CHECK_ARG(objectives);
    Y2_CHECK_ARG(opt && opt->size == (int)sizeof(yolo2_loss_options));
    return loss_impl(logits, ld, anchors, mask, prob, coords, off_min, off_max, areas, hparam, objectives, dlogits, ws, B, cell_h, cell_w, A, C, dtype, stream, *opt);
}
extern "C" int yolo2_loss_ex_partials(const void *logits, int ld, const float *anchors, const float *mask, const float *prob,
                                      const float *coords, const float *off_min, const float *off_max, const float *areas,
                                      const float *hparam, void *dlogits, float *ws, int B, int cell_h, int cell_w, int A, int C, int dtype,
                                      void *stream, const yolo2_loss_options *opt) {
    Y2_CHECK_ARG(opt && opt->size == (int)sizeof(yolo2_loss_options));
    return loss_impl(logits, ld, anchors, mask, prob, coords, off_min, off_max, areas, hparam, nullptr, dlogits, ws, B, cell_h, cell_w, A, C, dtype, stream, *opt);
}
extern "C" int yolo2_loss_objectives(const float *ws, float *objectives, int B, int cell_h, int cell_w, int A, void *stream) {
    Y2_CHECK_ARG(ws && objectives && B > 0 && cell_h > 0 && cell_w > 0 && A > 0 && A <= 64);
    const int nblocks = cdiv((long)B * cell_h * cell_w * lanes_per_cell(A), 256);
    loss_finalize_kernel<<<1, 256, 0, (hipStream_t)stream>>>(ws, nblocks, (float)((long)B * cell_h * cell_w * A), objectives);
    Y2_CHECK_LAUNCH();
    return YOLO2_OK;
}

// ------------------------------------------------------------------------------------------
// decode for detection (model/yolo2/__init__.py:50-56; calc_cell_xy model/yolo/__init__.py:29-34)
// ------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void decode_kernel(const T *__restrict__ logits, int ld, const float *__restrict__ anchors,
                                                     float *__restrict__ conf, float *__restrict__ xy_min, float *__restrict__ xy_max,
                                                     int *__restrict__ nan_flag, int B, int cell_h, int cell_w, int A, int C) {
    const int cells = cell_h * cell_w;
    const long total = (long)B * cells * A;
    const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= total) return;
    const int a = (int)(gid % A);
    const long cell_id = gid / A;
    const int cell = (int)(cell_id % cells);
    const float cx = (float)(cell % cell_w), cy = (float)(cell / cell_w);
    const int D = 5 + C;
    const T *lp = logits + cell_id * ld + a * D;
    const float s_iou = sigmoidf_((float)lp[0]);
    const float sx = sigmoidf_((float)lp[1]), sy = sigmoidf_((float)lp[2]);
    const float w = expf((float)lp[3]) * anchors[2 * a], h = expf((float)lp[4]) * anchors[2 * a + 1];
    const float hx = w / 2.0f, hy = h / 2.0f;
    float o[4] = {cx + (sx - hx), cy + (sy - hy), cx + (sx + hx), cy + (sy + hy)};
    xy_min[gid * 2] = o[0]; xy_min[gid * 2 + 1] = o[1];
    xy_max[gid * 2] = o[2]; xy_max[gid * 2 + 1] = o[3];
    bool bad = !(isfinite(o[0]) && isfinite(o[1]) && isfinite(o[2]) && isfinite(o[3]));
    float mx = -INFINITY;
    for (int k = 0; k < C; ++k) mx = fmaxf(mx, (float)lp[5 + k]);
    float den = 0.f;
    for (int k = 0; k < C; ++k) den += expf((float)lp[5 + k] - mx);
    for (int k = 0; k < C; ++k) {
        float v = s_iou * (expf((float)lp[5 + k] - mx) / den);
        conf[gid * C + k] = v;
        bad |= !isfinite(v);
    }
    if (bad && nan_flag) atomicOr(nan_flag, 1);
}

extern "C" int yolo2_head_decode(const void *logits, int ld, const float *anchors, float *conf, float *xy_min, float *xy_max,
                                 int *nan_flag, int B, int cell_h, int cell_w, int A, int C, int dtype, void *stream) {
    Y2_CHECK_ARG(logits && anchors && conf && xy_min && xy_max);
    Y2_CHECK_ARG(B > 0 && cell_h > 0 && cell_w > 0 && A > 0 && C > 0 && ld >= A * (5 + C));
    const long total = (long)B * cell_h * cell_w * A;
    Y2_DISPATCH_DTYPE(dtype, decode_kernel<T><<<cdiv(total, 256), 256, 0, (hipStream_t)stream>>>((const T *)logits, ld, anchors, conf, xy_min, xy_max, nan_flag, B, cell_h, cell_w, A, C));
    Y2_CHECK_LAUNCH();
    return YOLO2_OK;
}

// The remaining Model attributes reference callers read (demo_detect.py:62 uses prob, iou, xy_min, wh; model/yolo2/__init__.py:36-56):
// iou = sigmoid(ch 0), prob = softmax(classes), xy = cell_xy + sigmoid(ch 1:3), wh = exp(ch 3:5) * anchors.  Any output may be NULL.
template <typename T>
__global__ __launch_bounds__(256) void decode_attrs_kernel(const T *__restrict__ logits, int ld, const float *__restrict__ anchors, float *__restrict__ iou,
                                                           float *__restrict__ prob, float *__restrict__ xy, float *__restrict__ wh, int B, int cell_h,
                                                           int cell_w, int A, int C) {
    const int cells = cell_h * cell_w;
    const long total = (long)B * cells * A;
    const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= total) return;
    const int a = (int)(gid % A);
    const long cell_id = gid / A;
    const int cell = (int)(cell_id % cells);
    const T *lp = logits + cell_id * ld + a * (5 + C);
    if (iou) iou[gid] = sigmoidf_((float)lp[0]);
    if (xy) {
        xy[gid * 2] = (float)(cell % cell_w) + sigmoidf_((float)lp[1]);
        xy[gid * 2 + 1] = (float)(cell / cell_w) + sigmoidf_((float)lp[2]);
    }
    if (wh) {
        wh[gid * 2] = expf((float)lp[3]) * anchors[2 * a];
        wh[gid * 2 + 1] = expf((float)lp[4]) * anchors[2 * a + 1];
    }
    if (prob) {
        float mx = -INFINITY;
        for (int k = 0; k < C; ++k) mx = fmaxf(mx, (float)lp[5 + k]);
        float den = 0.f;
        for (int k = 0; k < C; ++k) den += expf((float)lp[5 + k] - mx);
        for (int k = 0; k < C; ++k) prob[gid * C + k] = expf((float)lp[5 + k] - mx) / den;
    }
}

extern "C" int yolo2_head_decode_attrs(const void *logits, int ld, const float *anchors, float *iou, float *prob, float *xy, float *wh,
                                       int B, int cell_h, int cell_w, int A, int C, int dtype, void *stream) {
    Y2_CHECK_ARG(logits && anchors && (iou || prob || xy || wh));
    Y2_CHECK_ARG(B > 0 && cell_h > 0 && cell_w > 0 && A > 0 && C > 0 && ld >= A * (5 + C));
    const long total = (long)B * cell_h * cell_w * A;
    Y2_DISPATCH_DTYPE(dtype, decode_attrs_kernel<T><<<cdiv(total, 256), 256, 0, (hipStream_t)stream>>>((const T *)logits, ld, anchors, iou, prob, xy, wh, B, cell_h, cell_w, A, C));
    Y2_CHECK_LAUNCH();
    return YOLO2_OK;
}
