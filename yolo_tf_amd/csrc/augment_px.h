// The per-pixel arithmetic of the input pipeline, shared by augment.hip (one source per output image) and compose.hip (mosaic / MixUp:
// several sources per output image): the bilinear sample of a crop, the TF-1.0 HSV pair, the photometric steps in the reference's order
// and the counter-based truncated normal.  f32 in the TF kernels' operation order; every unit that includes this is built with
// -ffp-contract=off, and the pragma below says so again for the functions themselves.
#pragma once
#include "common.h"
#pragma clang fp contract(off)

struct Px { float r, g, b; };

__device__ __forceinline__ Px rgb_to_hsv_tf(Px p) {
    const float v = fmaxf(fmaxf(p.r, p.g), p.b);
    const float range = v - fminf(fminf(p.r, p.g), p.b);
    const float s = v > 0.f ? range / v : 0.f;
    const float norm = 1.0f / (6.0f * range);
    float h;
    if (p.r == v) h = norm * (p.g - p.b);
    else if (p.g == v) h = norm * (p.b - p.r) + (float)(2.0 / 6.0);
    else h = norm * (p.r - p.g) + (float)(4.0 / 6.0);
    if (range <= 0.f) h = 0.f;
    if (h < 0.f) h = h + 1.0f;
    return Px{h, s, v};
}

__device__ __forceinline__ Px hsv_to_rgb_tf(Px q) {
    const float c = q.g * q.b;      // s * v
    const float m = q.b - c;
    const float dh = q.r * 6.0f;
    float fmodu = dh;
    while (fmodu <= 0.f) fmodu += 2.0f;
    while (fmodu >= 2.0f) fmodu -= 2.0f;
    const float x = c * (1.0f - fabsf(fmodu - 1.0f));
    const int cat = dh == 6.0f ? 5 : (int)dh;       // hue exactly 1.0 (h + 1 rounded up) is hue 0: sector 5 with x = 0
    float rr = 0.f, gg = 0.f, bb = 0.f;
    switch (cat) {
        case 0: rr = c; gg = x; break;
        case 1: rr = x; gg = c; break;
        case 2: gg = c; bb = x; break;
        case 3: gg = x; bb = c; break;
        case 4: rr = x; bb = c; break;
        case 5: rr = c; bb = x; break;
        default: break;
    }
    return Px{rr + m, gg + m, bb + m};
}

// The geometric part: pixel (y, x) of the crop (crop_x, crop_y, crop_w, crop_h) of `img` (rows of src_w pixels) resized to H x W
// (ResizeBilinear, align_corners=False; resize_images returns the input unchanged when the size matches).  The flip is the caller's.
__device__ __forceinline__ Px crop_resize_sample(const unsigned char *__restrict__ img, int src_w, int crop_x, int crop_y, int crop_w, int crop_h,
                                                 int y, int x, int H, int W) {
    const long row = (long)src_w * 3;
    if (crop_h == H && crop_w == W) {
        const unsigned char *t = img + (long)(crop_y + y) * row + (long)(crop_x + x) * 3;
        return Px{(float)t[0], (float)t[1], (float)t[2]};
    }
    const float hs = (float)crop_h / (float)H, ws = (float)crop_w / (float)W;
    const float fy = (float)y * hs, fx = (float)x * ws;
    const int y0 = (int)floorf(fy), x0 = (int)floorf(fx);
    const int y1 = min((int)ceilf(fy), crop_h - 1), x1 = min((int)ceilf(fx), crop_w - 1);
    const float ly = fy - (float)y0, lx = fx - (float)x0;
    const unsigned char *r0 = img + (long)(crop_y + y0) * row + (long)crop_x * 3;
    const unsigned char *r1 = img + (long)(crop_y + y1) * row + (long)crop_x * 3;
    float o[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float tl = (float)r0[x0 * 3 + c], tr = (float)r0[x1 * 3 + c];
        const float bl = (float)r1[x0 * 3 + c], br = (float)r1[x1 * 3 + c];
        const float top = tl + (tr - tl) * lx;
        const float bottom = bl + (br - bl) * lx;
        o[c] = top + (bottom - top) * ly;
    }
    return Px{o[0], o[1], o[2]};
}

// brightness, saturation, hue: the photometric steps before contrast (which needs the image's mean of this value)
__device__ __forceinline__ Px photo_before_contrast(Px v, const yolo2_augment_params &p) {
    if (p.flags & YOLO2_AUG_BRIGHTNESS) { v.r += p.brightness; v.g += p.brightness; v.b += p.brightness; }
    if (p.flags & YOLO2_AUG_SATURATION) {
        Px q = rgb_to_hsv_tf(v);
        q.g = fminf(fmaxf(q.g * p.saturation, 0.f), 1.f);
        v = hsv_to_rgb_tf(q);
    }
    if (p.flags & YOLO2_AUG_HUE) {
        Px q = rgb_to_hsv_tf(v);
        float h = q.r + (1.0f + p.hue);
        h = h - floorf(h);                           // floormod(h, 1)
        q.r = h;
        v = hsv_to_rgb_tf(q);
    }
    return v;
}

__device__ __forceinline__ unsigned hash32(unsigned x) {       // "lowbias32" integer finaliser
    x ^= x >> 16; x *= 0x7feb352du;
    x ^= x >> 15; x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}
// Three standard normals truncated to |z| <= 2 by resampling (tf.truncated_normal), counter-based on (seed, pixel):
// two Box-Muller pairs per pixel from four 24-bit uniforms; a component beyond 2 sigma (4.6 %) is redrawn on its own
// counter stream.  Fast-math log / sincos: this is noise, not parity arithmetic.
__device__ __forceinline__ void box_muller(unsigned a, unsigned b, float &z0, float &z1) {
    const float u1 = ((float)(a >> 8) + 1.0f) * (1.0f / 16777216.0f);      // (0, 1]
    const float u2 = (float)(b >> 8) * (1.0f / 16777216.0f);               // [0, 1)
    const float r = sqrtf(-2.0f * __logf(u1));
    float sn, cs;
    __sincosf(6.28318530717958647692f * u2, &sn, &cs);
    z0 = r * cs;
    z1 = r * sn;
}
__device__ __forceinline__ void truncated_normal3(unsigned long long seed, unsigned pixel, float (&z)[3]) {
    const unsigned s0 = (unsigned)seed, s1 = (unsigned)(seed >> 32);
    const unsigned base = hash32(pixel ^ s0) + s1;
    float t[4];
    box_muller(hash32(base), hash32(base + 0x9e3779b9u), t[0], t[1]);
    box_muller(hash32(base + 0x3c6ef372u), hash32(base + 0xdaa66d2bu), t[2], t[3]);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float v = t[c];
        if (fabsf(v) > 2.0f) {
            v = fabsf(t[3]) <= 2.0f && c == 0 ? t[3] : 3.0f;           // the spare fourth sample serves the first reject
            unsigned ctr = hash32(base ^ (0x85ebca6bu * (unsigned)(c + 1)));
            for (int attempt = 0; attempt < 32 && fabsf(v) > 2.0f; ++attempt) {
                float w;
                box_muller(hash32(ctr), hash32(ctr + 0x9e3779b9u), v, w);
                if (fabsf(v) > 2.0f) v = w;
                ctr += 0x632be5abu;
            }
            if (fabsf(v) > 2.0f) v = 0.f;
        }
        z[c] = v;
    }
}

// contrast about `mean`, noise indexed by the output pixel, grey, clip, store: everything after photo_before_contrast
__device__ __forceinline__ void finish_and_store(Px v, const yolo2_augment_params &p, const float (&mean)[3], unsigned pixel, float *__restrict__ o) {
    if (p.flags & YOLO2_AUG_CONTRAST) {
        v.r = (v.r - mean[0]) * p.contrast + mean[0];
        v.g = (v.g - mean[1]) * p.contrast + mean[1];
        v.b = (v.b - mean[2]) * p.contrast + mean[2];
    }
    if (p.flags & YOLO2_AUG_NOISE) {
        float z[3];
        truncated_normal3(p.noise_seed, pixel, z);
        v.r = v.r + z[0] * p.noise_scale;
        v.g = v.g + z[1] * p.noise_scale;
        v.b = v.b + z[2] * p.noise_scale;
    }
    if (p.flags & YOLO2_AUG_GRAY) {
        const float g = (v.r * 0.2989f + v.g * 0.5870f) + v.b * 0.1140f;
        v = Px{g, g, g};
    }
    o[0] = fminf(fmaxf(v.r, 0.f), 255.f);
    o[1] = fminf(fmaxf(v.g, 0.f), 255.f);
    o[2] = fminf(fmaxf(v.b, 0.f), 255.f);
}

// the per-channel means of AdjustContrastv2 from pass A's f64 sums; zero for an image without the flag
__device__ __forceinline__ void contrast_means(const yolo2_augment_params &p, const double *__restrict__ sums, int b, int total, float (&mean)[3]) {
    mean[0] = mean[1] = mean[2] = 0.f;
    if (p.flags & YOLO2_AUG_CONTRAST) {
#pragma unroll
        for (int c = 0; c < 3; ++c) mean[c] = (float)(sums[3 * b + c] / (double)total);
    }
}

// one wave's share of pass A into the image's three f64 sums
__device__ __forceinline__ void add_channel_sums(double (&s)[3], double *__restrict__ sums, int b) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double t = wave_sum_d(s[c]);
        if ((threadIdx.x & 63) == 0) atomicAdd(sums + 3 * b + c, t);
    }
}
