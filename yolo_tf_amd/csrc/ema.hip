// Exponential moving average of the parameter arena (tf.train.ExponentialMovingAverage's assign_moving_average), gfx950.
// Built with -ffp-contract=off: the three operations of an element are rounded one by one, as the NumPy specification (tests/ema_ref.py) does.
#include "common.h"

// [TF-sem] assign_moving_average: variable -= (variable - value) * (1 - decay)
__device__ __forceinline__ float ema_one(float e, float w, float omd) {
    float d = e - w;
    d = d * omd;
    return e - d;
}
// 12 B of HBM traffic per element.  `head` scalar elements bring ema to a 16-byte boundary; the body takes 16-byte accesses when w is aligned there
// as well (the arenas are; slices with different misalignments are not, and run scalar: the host passes head = n), a scalar tail ends it.
__global__ __launch_bounds__(256) void ema_kernel(float *__restrict__ ema, const float *__restrict__ w, long n, long head, float omd) {
    const long stride = (long)gridDim.x * blockDim.x;
    const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
    for (long k = i; k < head; k += stride) ema[k] = ema_one(ema[k], w[k], omd);
    const long n4 = (n - head) >> 2;
    f32x4 *e4 = reinterpret_cast<f32x4 *>(ema + head);
    const f32x4 *w4 = reinterpret_cast<const f32x4 *>(w + head);
    for (long k = i; k < n4; k += stride) {
        f32x4 ev = e4[k];
        const f32x4 wv = w4[k];
#pragma unroll
        for (int j = 0; j < 4; ++j) ev[j] = ema_one(ev[j], wv[j], omd);
        e4[k] = ev;
    }
    for (long k = head + (n4 << 2) + i; k < n; k += stride) ema[k] = ema_one(ema[k], w[k], omd);
}

extern "C" int yolo2_ema_update(float *ema, const float *w, long n, float one_minus_decay, void *stream) {
    Y2_CHECK_ARG(ema && w && n > 0 && one_minus_decay >= 0 && one_minus_decay <= 1);
    Y2_CHECK_ARG((((uintptr_t)ema) | ((uintptr_t)w)) % sizeof(float) == 0);
    // elements in front of ema's first 16-byte boundary; everything when w is not on one at the same element
    long head = (long)(((16 - ((uintptr_t)ema & 15)) & 15) / sizeof(float));
    if (head > n || (((uintptr_t)(w + head)) & 15) != 0) head = n;
    // memory-bound: eight 256-thread workgroups per CU, the grid-stride loop takes the rest
    long blocks = ((n - head) / 4 + 255) / 256;
    if (blocks < (head + 255) / 256) blocks = (head + 255) / 256;
    const long cap = 8L * y2_device_cus();
    if (blocks > cap) blocks = cap;
    if (blocks < 1) blocks = 1;
    ema_kernel<<<(int)blocks, 256, 0, (hipStream_t)stream>>>(ema, w, n, head, one_minus_decay);
    Y2_CHECK_LAUNCH();
    return YOLO2_OK;
}
