// On-device input pipeline: the image half of load_image_labels (reference
// utils/data/__init__.py:162-175) after JPEG decode -- crop_to_bounding_box -> resize_images (bilinear) -> flip ->
// brightness -> saturation -> hue -> contrast -> noise -> grayscale -> clip -- and transform_labels
// (utils/data/__init__.py:112-145), so a training step consumes decoded uint8 images and raw boxes resident in HBM
// instead of a host-side TF queue.
//
// Every random decision of the reference (tf.random_uniform / tf.cond / truncated_normal's scale) is drawn on the
// host and arrives in yolo2_augment_params; only the per-pixel noise is generated here (counter-based hash ->
// Box-Muller, resampled to |z| <= 2 like tf.truncated_normal).  The image arithmetic restates the TF-1.0 kernels in
// f32 in their operation order (ResizeBilinear align_corners=False, RGBToHSV / HSVToRGB, AdjustContrastv2,
// rgb_to_grayscale weights); oracle/yolo2_ref.py holds the same restatement (parity unpinned by the reference: the
// arithmetic lives in TensorFlow).  One point departs from a literal reading of HSVToRGB's switch: rgb_to_hsv wraps a
// negative hue with h + 1, which for |h| < 2^-25 rounds to exactly 1.0f; dh is then 6 and a literal switch falls to its
// default and returns (m, m, m), losing the dominant channel.  Hue is periodic, so dh == 6 is treated as sector 5 here
// and in the oracle (fmodu is 0 there: (c + m, m, m), the value at hue 0).
// The per-pixel arithmetic itself is in augment_px.h.  HBM-bound: one uint8 source read (4 taps, L2-resident) + one f32 write per pixel;
// contrast needs the per-channel image mean of the value BEFORE contrast, so images that take that branch are
// evaluated twice (pass A: sums, pass B: output) rather than staged.
#include "augment_px.h"      // the per-pixel arithmetic, shared with compose.hip
#pragma clang fp contract(off)

// value of output pixel (y, x) after crop, resize, flip, brightness, saturation, hue (everything before contrast)
__device__ __forceinline__ Px pixel_before_contrast(const unsigned char *__restrict__ src, const yolo2_augment_params &p, int y, int x, int H, int W) {
    if (p.flags & YOLO2_AUG_FLIP) x = W - 1 - x;
    const Px v = crop_resize_sample(src + p.src_offset, p.src_w, p.crop_x, p.crop_y, p.crop_w, p.crop_h, y, x, H, W);
    return photo_before_contrast(v, p);
}

// pass A: per image, per channel sums of the pre-contrast value (only images with the contrast flag do work)
__global__ __launch_bounds__(256) void augment_sums_kernel(const unsigned char *__restrict__ src, const yolo2_augment_params *__restrict__ params,
                                                           double *__restrict__ sums, int H, int W) {
    const int b = blockIdx.y;
    const yolo2_augment_params p = params[b];
    if (!(p.flags & YOLO2_AUG_CONTRAST)) return;
    double s[3] = {0.0, 0.0, 0.0};
    const int total = H * W;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const Px v = pixel_before_contrast(src, p, i / W, i % W, H, W);
        s[0] += (double)v.r;
        s[1] += (double)v.g;
        s[2] += (double)v.b;
    }
    add_channel_sums(s, sums, b);
}

// pass B: the whole chain, f32 [B, H, W, 3] out
__global__ __launch_bounds__(256) void augment_apply_kernel(const unsigned char *__restrict__ src, const yolo2_augment_params *__restrict__ params,
                                                            const double *__restrict__ sums, float *__restrict__ out, int H, int W) {
    const int b = blockIdx.y;
    const yolo2_augment_params p = params[b];
    const int total = H * W;
    float mean[3];
    contrast_means(p, sums, b, total, mean);
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const Px v = pixel_before_contrast(src, p, i / W, i % W, H, W);
        finish_and_store(v, p, mean, (unsigned)i, out + ((long)b * total + i) * 3);
    }
}

// bytes of the caller-owned scratch `ws` below: three doubles per image
extern "C" size_t yolo2_augment_workspace_bytes(int B) { return (size_t)3 * (size_t)(B > 0 ? B : 0) * sizeof(double); }
extern "C" int yolo2_augment_images(const unsigned char *src, const yolo2_augment_params *params_device, double *ws, float *out, int B, int H,
                                    int W, int any_contrast, void *stream) {
    Y2_CHECK_ARG(src && params_device && out && B > 0 && H > 0 && W > 0);
    Y2_CHECK_ARG(!any_contrast || ws);
    hipStream_t st = (hipStream_t)stream;
    const int bx = B >= 64 ? 8 : B >= 8 ? 32 : 128;
    dim3 grid(bx, B);
    if (any_contrast) {
        if (hipMemsetAsync(ws, 0, sizeof(double) * 3 * B, st) != hipSuccess) { yolo2_set_error("yolo2_augment_images: memset failed"); return YOLO2_E_LAUNCH; }
        augment_sums_kernel<<<grid, 256, 0, st>>>(src, params_device, ws, H, W);
    }
    augment_apply_kernel<<<grid, 256, 0, st>>>(src, params_device, ws, out, H, W);
    Y2_CHECK_LAUNCH();
    return YOLO2_OK;
}

// ---------------------------------------------------------------------------------------------------------
// transform_labels (utils/data/__init__.py:112-145): boxes normalised to [0,1] -> the six label tensors of the loss.
// One workgroup per image: all threads clear the image's slices, then one lane replays the objects IN ORDER (NumPy
// fancy assignment with repeated indices: the last object of a cell wins for coords / offsets, class bits accumulate),
// f32 arithmetic in NumPy's operation order with contraction off -> bit-exact against the reference's goldens.
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void transform_labels_kernel(const int *__restrict__ cls, const float *__restrict__ box, const int *__restrict__ first,
                                                               float *__restrict__ mask, float *__restrict__ prob, float *__restrict__ coords,
                                                               float *__restrict__ off_min, float *__restrict__ off_max, float *__restrict__ areas,
                                                               int classes, int cell_w, int cell_h, int *__restrict__ err) {
    const int b = blockIdx.x, cells = cell_w * cell_h;
    float *m = mask + (long)b * cells, *pr = prob + (long)b * cells * classes, *co = coords + (long)b * cells * 4;
    float *mn = off_min + (long)b * cells * 2, *mx = off_max + (long)b * cells * 2, *ar = areas + (long)b * cells;
    for (int i = threadIdx.x; i < cells; i += blockDim.x) m[i] = 0.f;
    for (int i = threadIdx.x; i < cells * classes; i += blockDim.x) pr[i] = 0.f;
    for (int i = threadIdx.x; i < cells * 4; i += blockDim.x) co[i] = 0.f;
    for (int i = threadIdx.x; i < cells * 2; i += blockDim.x) { mn[i] = 0.f; mx[i] = 0.f; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const float cw = (float)cell_w, ch = (float)cell_h;
        for (int k = first[b]; k < first[b + 1]; ++k) {
            const float xmin = box[4 * k], ymin = box[4 * k + 1], xmax = box[4 * k + 2], ymax = box[4 * k + 3];
            const float x = cw * (xmin + xmax) / 2.0f, y = ch * (ymin + ymax) / 2.0f;
            const float ix = floorf(x), iy = floorf(y);
            const float ox = x - ix, oy = y - iy;
            const float w = xmax - xmin, h = ymax - ymin;
            const int index = (int)(iy * cw + ix);
            const int c = cls[k];
            if (index < 0 || index >= cells || c < 0 || c >= classes) { atomicOr(err, 1); continue; }   // the reference raises IndexError
            m[index] = 1.f;
            pr[(long)index * classes + c] = 1.f;
            co[index * 4 + 0] = ox;
            co[index * 4 + 1] = oy;
            co[index * 4 + 2] = (float)sqrt((double)w);      // correctly rounded f32 square root (np.sqrt): via f64, 53 >= 2*24+2
            co[index * 4 + 3] = (float)sqrt((double)h);
            const float hw = w / 2.0f * cw, hh = h / 2.0f * ch;
            mn[index * 2 + 0] = ox - hw;
            mn[index * 2 + 1] = oy - hh;
            mx[index * 2 + 0] = ox + hw;
            mx[index * 2 + 1] = oy + hh;
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < cells; i += blockDim.x) {
        const float ew = mx[i * 2] - mn[i * 2], eh = mx[i * 2 + 1] - mn[i * 2 + 1];
        if (ew < 0.f || eh < 0.f) atomicOr(err, 2);          // the reference asserts wh >= 0
        ar[i] = ew * eh;
    }
}

extern "C" int yolo2_transform_labels(const int *objects_class, const float *objects_coord, const int *first_object, float *mask, float *prob,
                                      float *coords, float *offset_xy_min, float *offset_xy_max, float *areas, int B, int classes, int cell_width,
                                      int cell_height, int *error_flag, void *stream) {
    Y2_CHECK_ARG(objects_class && objects_coord && first_object && mask && prob && coords && offset_xy_min && offset_xy_max && areas && error_flag);
    Y2_CHECK_ARG(B > 0 && classes > 0 && cell_width > 0 && cell_height > 0);
    transform_labels_kernel<<<B, 256, 0, (hipStream_t)stream>>>(objects_class, objects_coord, first_object, mask, prob, coords, offset_xy_min,
                                                                offset_xy_max, areas, classes, cell_width, cell_height, error_flag);
    Y2_CHECK_LAUNCH();
    return YOLO2_OK;
}
