// Mosaic and MixUp for the on-device input pipeline (new work, the reference has neither): an output image is
// composed of up to two layers of up to four tiles, each tile a crop of its own source resized to a view of its own size and placed
// anywhere on the frame; the photometric chain of augment.hip then runs once on the composite.  The per-pixel arithmetic is
// augment_px.h's, shared with augment.hip: one full-frame tile reproduces yolo2_augment_images bit for bit.
//
// Work is handed out by PIECE, not by pixel: a piece is the intersection of one tile's rectangle of layer 0 with one of layer 1 (or the
// tile's rectangle itself when there is no second layer), at most 16 per image, enumerated by loops every lane of the grid takes
// alike.  The tile records are therefore indexed by block-uniform values only and arrive through scalar loads; no lane searches
// the table for its pixel.  The lanes run one grid-stride index through the concatenated pieces (j carries over from piece to piece),
// so a 2x2 mosaic takes the trips its pixel count needs, not one ragged tail per piece.  A single full-frame tile is one piece whose
// index is the flat pixel index: the loop of augment.hip.
// HBM-bound like augment.hip: 12 B written per pixel, at most four byte taps (L2-resident) read per layer; an image with the contrast
// flag is evaluated twice (pass A: f64 sums of the composite, pass B: output).
#include "augment_px.h"
#pragma clang fp contract(off)

// the tile's contribution to output pixel (y, x): the view's sample, or `fill` outside the view
__device__ __forceinline__ Px tile_pixel(const unsigned char *__restrict__ src, const yolo2_compose_tile &t, int y, int x, float fill) {
    int u = x - t.origin_x;
    const int v = y - t.origin_y;
    if (u < 0 || u >= t.view_w || v < 0 || v >= t.view_h) return Px{fill, fill, fill};
    if (t.flip) u = t.view_w - 1 - u;
    return crop_resize_sample(src + t.src_offset, t.src_w, t.crop_x, t.crop_y, t.crop_w, t.crop_h, v, u, t.view_h, t.view_w);
}

// Calls f(y, x, value before contrast) for this lane's share of image b's pixels.
template <typename F>
__device__ __forceinline__ void for_each_composite_pixel(const unsigned char *__restrict__ src, const yolo2_compose_tile *__restrict__ tiles,
                                                         const yolo2_augment_params &p, float lam, bool two, int b, int L, int T, int H, int W,
                                                         float fill, F f) {
    const yolo2_compose_tile *t0s = tiles + (long)b * L * T, *t1s = t0s + T;
    const int stride = gridDim.x * blockDim.x;
    int j = blockIdx.x * blockDim.x + threadIdx.x;          // position in the concatenation of the pieces still ahead
    for (int k0 = 0; k0 < T; ++k0) {
        const yolo2_compose_tile t0 = t0s[k0];
        const int ax0 = max(t0.x0, 0), ay0 = max(t0.y0, 0), ax1 = min(t0.x1, W), ay1 = min(t0.y1, H);      // never a pixel outside the frame
        if (ax1 <= ax0 || ay1 <= ay0) continue;              // an unused slot
        for (int k1 = 0; k1 < (two ? T : 1); ++k1) {
            yolo2_compose_tile t1 = t0;
            int px0 = ax0, py0 = ay0, px1 = ax1, py1 = ay1;
            if (two) {
                t1 = t1s[k1];
                px0 = max(px0, t1.x0); py0 = max(py0, t1.y0); px1 = min(px1, t1.x1); py1 = min(py1, t1.y1);
                if (px1 <= px0 || py1 <= py0) continue;
            }
            const int pw = px1 - px0, n = pw * (py1 - py0);
            for (; j < n; j += stride) {
                const int y = py0 + j / pw, x = px0 + j % pw;
                Px v = tile_pixel(src, t0, y, x, fill);
                if (two) {
                    const Px w = tile_pixel(src, t1, y, x, fill);
                    v.r = v.r * lam + w.r * (1.0f - lam);
                    v.g = v.g * lam + w.g * (1.0f - lam);
                    v.b = v.b * lam + w.b * (1.0f - lam);
                }
                f(y, x, photo_before_contrast(v, p));
            }
            j -= n;
        }
    }
}

// pass A: per image, per channel sums of the composite before contrast (only images with the contrast flag do work)
__global__ __launch_bounds__(256) void compose_sums_kernel(const unsigned char *__restrict__ src, const yolo2_compose_tile *__restrict__ tiles,
                                                           const yolo2_augment_params *__restrict__ photo, const float *__restrict__ mix,
                                                           double *__restrict__ sums, int L, int T, int H, int W, float fill) {
    const int b = blockIdx.y;
    const yolo2_augment_params p = photo[b];
    if (!(p.flags & YOLO2_AUG_CONTRAST)) return;
    const float lam = L == 2 ? mix[b] : 1.0f;
    double s[3] = {0.0, 0.0, 0.0};
    for_each_composite_pixel(src, tiles, p, lam, L == 2 && lam != 1.0f, b, L, T, H, W, fill, [&](int, int, Px v) {
        s[0] += (double)v.r;
        s[1] += (double)v.g;
        s[2] += (double)v.b;
    });
    add_channel_sums(s, sums, b);
}

// pass B: the whole chain, f32 [B, H, W, 3] out
__global__ __launch_bounds__(256) void compose_apply_kernel(const unsigned char *__restrict__ src, const yolo2_compose_tile *__restrict__ tiles,
                                                            const yolo2_augment_params *__restrict__ photo, const float *__restrict__ mix,
                                                            const double *__restrict__ sums, float *__restrict__ out, int L, int T, int H, int W,
                                                            float fill) {
    const int b = blockIdx.y;
    const yolo2_augment_params p = photo[b];
    const int total = H * W;
    const float lam = L == 2 ? mix[b] : 1.0f;
    float mean[3];
    contrast_means(p, sums, b, total, mean);
    float *o = out + (long)b * total * 3;
    for_each_composite_pixel(src, tiles, p, lam, L == 2 && lam != 1.0f, b, L, T, H, W, fill, [&](int y, int x, Px v) {
        const int i = y * W + x;
        finish_and_store(v, p, mean, (unsigned)i, o + (long)i * 3);
    });
}

extern "C" int yolo2_compose_images(const unsigned char *src, const yolo2_compose_tile *tiles, const yolo2_augment_params *photo, const float *mix,
                                    double *ws, float *out, int B, int L, int T, int H, int W, float fill, int any_contrast, void *stream) {
    Y2_CHECK_ARG(src && tiles && photo && out && B > 0 && H > 0 && W > 0);
    Y2_CHECK_ARG(L == 1 || L == 2);
    Y2_CHECK_ARG(T >= 1 && T <= 4);
    Y2_CHECK_ARG(L == 1 || mix);
    Y2_CHECK_ARG(!any_contrast || ws);
    Y2_CHECK_ARG((long)H * W < (1L << 30));      // the pixel index and its grid stride stay inside an int
    hipStream_t st = (hipStream_t)stream;
    const int bx = B >= 64 ? 8 : B >= 8 ? 32 : 128;          // yolo2_augment_images' grid
    dim3 grid(bx, B);
    if (any_contrast) {
        if (hipMemsetAsync(ws, 0, sizeof(double) * 3 * B, st) != hipSuccess) { yolo2_set_error("yolo2_compose_images: memset failed"); return YOLO2_E_LAUNCH; }
        compose_sums_kernel<<<grid, 256, 0, st>>>(src, tiles, photo, mix, ws, L, T, H, W, fill);
    }
    compose_apply_kernel<<<grid, 256, 0, st>>>(src, tiles, photo, mix, ws, out, L, T, H, W, fill);
    Y2_CHECK_LAUNCH();
    return YOLO2_OK;
}
