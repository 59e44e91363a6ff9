// IoU-family box regression scores for the YOLOv2 loss (head.hip: loss_kernel<T, MODE>, MODE != mse): IoU, GIoU (Rezatofighi et al.,
// CVPR 2019), DIoU and CIoU (Zheng et al., AAAI 2020) of one predicted box against its cell's target, with the closed-form derivative with
// respect to (sx, sy, w, h).  The frame is the one the matching IoU uses: cell units relative to the cell.  tests/box_loss_ref.py is the
// specification; only the responsible lanes of a launch come here, a handful per image.
//
// Kink conventions: at an exact tie of a predicted and a target edge the derivative goes to the predicted edge; max(., 0) and the 1e-10
// floors have zero derivative where they clamp.  The CIoU weight alpha is a constant in the derivative (as in the paper); the derivative
// of v is the true one, with its 1 / (w^2 + h^2) factor (w^2 + h^2 floored at 1e-30, against underflow).
#pragma once

enum { Y2_BOX_MSE = 0, Y2_BOX_IOU = 1, Y2_BOX_GIOU = 2, Y2_BOX_DIOU = 3, Y2_BOX_CIOU = 4, Y2_BOX_MODES = 5 };

// d sigmoid(z) / dz = e / (1 + e)^2 with e = exp(-|z|): unlike s * (1 - s) it keeps its relative accuracy where the sigmoid saturates
__device__ __forceinline__ float dsigmoidf_(float z) {
    const float e = expf(-fabsf(z));
    return e / ((1.0f + e) * (1.0f + e));
}

// Returns the score q (the objective is 1 - q); g = dq / d(sx, sy, w, h).  Predicted box: centre (sx, sy), size (w, h); target: edges
// (X1, Y1)-(X2, Y2) and the area label At.  I, U and the IoU are formed exactly as the matching IoU of loss_kernel forms them.
template <int MODE>
__device__ __forceinline__ float box_score(float sx, float sy, float w, float h, float X1, float Y1, float X2, float Y2, float At, float g[4]) {
    const float hx = w / 2.0f, hy = h / 2.0f;
    const float x1 = sx - hx, y1 = sy - hy, x2 = sx + hx, y2 = sy + hy;
    const float rx = fminf(x2, X2) - fmaxf(x1, X1), ry = fminf(y2, Y2) - fmaxf(y1, Y1);
    const float ix = fmaxf(rx, 0.0f), iy = fmaxf(ry, 0.0f);
    const float inter = ix * iy;
    const float uraw = (At + w * h) - inter;
    const float uni = fmaxf(uraw, 1e-10f);
    const float iou = inter / uni;
    // the intersection's edges that belong to the predicted box (ties included), where the intersection is not empty
    const float lx = rx > 0.0f ? 1.0f : 0.0f, ly = ry > 0.0f ? 1.0f : 0.0f;
    const float ax1 = x1 >= X1 ? lx : 0.0f, ax2 = x2 <= X2 ? lx : 0.0f, ay1 = y1 >= Y1 ? ly : 0.0f, ay2 = y2 <= Y2 ? ly : 0.0f;
    float dI[4] = {iy * (ax2 - ax1), ix * (ay2 - ay1), iy * (ax2 + ax1) * 0.5f, ix * (ay2 + ay1) * 0.5f};
    const float uf = uraw > 1e-10f ? 1.0f : 0.0f;
    float dU[4] = {-uf * dI[0], -uf * dI[1], uf * (h - dI[2]), uf * (w - dI[3])};
#pragma unroll
    for (int k = 0; k < 4; ++k) g[k] = (dI[k] - iou * dU[k]) / uni;
    float q = iou;
    if constexpr (MODE >= Y2_BOX_GIOU) {
        // the enclosing box and the edges of it that belong to the predicted box (ties included)
        const float ew = fmaxf(x2, X2) - fminf(x1, X1), eh = fmaxf(y2, Y2) - fminf(y1, Y1);
        const float bx1 = x1 <= X1 ? 1.0f : 0.0f, bx2 = x2 >= X2 ? 1.0f : 0.0f, by1 = y1 <= Y1 ? 1.0f : 0.0f, by2 = y2 >= Y2 ? 1.0f : 0.0f;
        const float dew[4] = {bx2 - bx1, 0.0f, (bx2 + bx1) * 0.5f, 0.0f}, deh[4] = {0.0f, by2 - by1, 0.0f, (by2 + by1) * 0.5f};
        if constexpr (MODE == Y2_BOX_GIOU) {
            const float eraw = ew * eh;
            const float enc = fmaxf(eraw, 1e-10f);
            const float ef = eraw > 1e-10f ? 1.0f : 0.0f;
            const float r = uni / enc;
            q = iou - (enc - uni) / enc;
#pragma unroll
            for (int k = 0; k < 4; ++k) g[k] += (dU[k] - r * (ef * (eh * dew[k] + ew * deh[k]))) / enc;
        } else {
            const float dx = sx - (X1 + X2) / 2.0f, dy = sy - (Y1 + Y2) / 2.0f;
            const float rho2 = dx * dx + dy * dy;
            const float craw = ew * ew + eh * eh;
            const float c2 = fmaxf(craw, 1e-10f);
            const float cf = craw > 1e-10f ? 2.0f : 0.0f;
            const float pen = rho2 / c2;
            q = iou - pen;
            const float drho[4] = {2.0f * dx, 2.0f * dy, 0.0f, 0.0f};
#pragma unroll
            for (int k = 0; k < 4; ++k) g[k] -= (drho[k] - pen * (cf * (ew * dew[k] + eh * deh[k]))) / c2;
            if constexpr (MODE == Y2_BOX_CIOU) {
                const float k4 = 0.40528473456935109f;      // 4 / pi^2
                const float dth = atan2f(X2 - X1, Y2 - Y1) - atan2f(w, h);
                const float v = k4 * (dth * dth);
                const float alpha = v / ((1.0f - iou) + v + 1e-10f);
                q -= alpha * v;
                // alpha * dv/d(theta_p) = -2 k4 dth, over w^2 + h^2.  Floored at 1e-30, where only underflow reaches it (exp giving a 0 x 0 box must not
                // put NaN in dlogits); not at 1e-10 like the forward's floors: the factor is the derivative's own and a 1e-5-cell box is still a box
                const float t = alpha * (2.0f * k4) * dth / fmaxf(w * w + h * h, 1e-30f);
                g[2] += t * h;       // d theta_p / dw =  h / (w^2 + h^2)
                g[3] -= t * w;       // d theta_p / dh = -w / (w^2 + h^2)
            }
        }
    }
    return q;
}
