// Device code the two evaluators (eval.hip: PASCAL VOC, eval_coco.hip: COCO) share: the order key of a score, the f32 IoU, how a
// score row becomes detections, and the LSD radix passes over 16-byte records (histogram per 16384-record tile, one-workgroup scan of
// the digit x tile table, stable scatter).  The passes are templated on a field functor F:
//   F::get(r, field, C)            the 32-bit sort field `field` of record r
//   F::bad(r, n_images, N, C)      true when r names something outside what finalize was told (checked by the first pass only)
#pragma once
#include "common.h"
#pragma clang fp contract(off)

#define EV_TILE_ITEMS 64
#define EV_TILE (256 * EV_TILE_ITEMS)       // records per workgroup of a radix pass
#define EV_ERR_GT_CLASS 1ull                 // a ground truth class id outside [0, C)
#define EV_ERR_GT_FIRST 2ull                 // gt_first not ascending inside [0, G], or more than YOLO2_EVAL_MAX_GT_PER_IMAGE boxes in an image
#define EV_ERR_RECORD 4ull                   // a record's image / box index outside what finalize was told

__device__ __forceinline__ unsigned ev_ord(float s) {        // ascending in this <=> ascending score
    const unsigned b = __builtin_bit_cast(unsigned, s);
    return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ __forceinline__ float ev_unord(unsigned o) {      // the inverse of ev_ord
    const unsigned b = o ^ ((o >> 31) ? 0x80000000u : 0xFFFFFFFFu);
    return __builtin_bit_cast(float, b);
}
__device__ __forceinline__ float ev_iou(const f32x4 p, const f32x4 q) {
    const float a1 = (p[2] - p[0]) * (p[3] - p[1]);
    const float a2 = (q[2] - q[0]) * (q[3] - q[1]);
    const float w = fmaxf(fminf(p[2], q[2]) - fmaxf(p[0], q[0]), 0.0f);
    const float h = fmaxf(fminf(p[3], q[3]) - fmaxf(p[1], q[1]), 0.0f);
    const float inter = w * h;
    return inter / fmaxf((a1 + a2) - inter, 1e-10f);
}
// item `it` of image row `conf` -> is it a detection, and which (box, class, score)
__device__ __forceinline__ bool ev_item(const float *__restrict__ conf, int it, int items, int C, float thr, int mode, int &box, int &cls, float &score) {
    if (it >= items) return false;
    if (mode == YOLO2_EVAL_MODE_ALL) {
        box = it / C;
        cls = it - box * C;
        score = conf[it] + 0.0f;                         // (-0 -> +0: one bit pattern per value, the order key is the bits)
        return score > thr;
    }
    box = it;
    const float *row = conf + (long)it * C;
    float best = row[0];
    bool nan = best != best;
    int arg = 0;
    for (int c = 1; c < C; ++c) {
        const float v = row[c];
        nan |= v != v;
        if (v > best) { best = v; arg = c; }           // strict: the FIRST arg-max
    }
    cls = arg;
    score = best + 0.0f;
    return !nan && score > thr;
}
__device__ __forceinline__ int ev_block_sum(int v, int *sred) {      // 256 threads; every thread gets the sum
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sred[threadIdx.x >> 6] = v;
    __syncthreads();
    return sred[0] + sred[1] + sred[2] + sred[3];
}
__device__ __forceinline__ long ev_count(const unsigned long long *state, long capacity) {
    const unsigned long long n = state[0];
    return n < (unsigned long long)capacity ? (long)n : capacity;
}

template <class F>
__global__ __launch_bounds__(256) void eval_hist_kernel(const u32x4 *__restrict__ src, unsigned long long *__restrict__ state, long capacity,
                                                        int *__restrict__ table, int field, int shift, int C, int check, int n_images, int N) {
    __shared__ int h[256];
    const long M = ev_count(state, capacity);
    const long lo = (long)blockIdx.x * EV_TILE, hi = min(lo + EV_TILE, M);
    h[threadIdx.x] = 0;
    __syncthreads();
    bool bad = false;
    for (long i = lo + threadIdx.x; i < hi; i += 256) {
        const u32x4 r = src[i];
        atomicAdd(&h[(F::get(r, field, C) >> shift) & 255u], 1);
        if (check) bad |= F::bad(r, n_images, N, C);
    }
    if (bad) atomicOr(&state[1], EV_ERR_RECORD);
    __syncthreads();
    table[(long)blockIdx.x * 256 + threadIdx.x] = h[threadIdx.x];
}

// table[tile][digit] counts -> start positions, ordered digit-major, tile-minor
static __global__ __launch_bounds__(256) void eval_scan_kernel(int *__restrict__ table, int tiles) {
    __shared__ int tot[256];
    const int d = threadIdx.x;
    int s = 0;
    for (int j = 0; j < tiles; ++j) s += table[(long)j * 256 + d];
    tot[d] = s;
    __syncthreads();
    int off = 0;
    for (int k = 0; k < d; ++k) off += tot[k];
    for (int j = 0; j < tiles; ++j) {
        const int v = table[(long)j * 256 + d];
        table[(long)j * 256 + d] = off;
        off += v;
    }
}

template <class F>
__global__ __launch_bounds__(256) void eval_scatter_kernel(const u32x4 *__restrict__ src, u32x4 *__restrict__ dst, const unsigned long long *__restrict__ state,
                                                           long capacity, const int *__restrict__ table, int field, int shift, int C) {
    __shared__ int base[256];
    __shared__ int wcnt[4][256];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long M = ev_count(state, capacity);
    const long lo = (long)blockIdx.x * EV_TILE;
    if (lo >= M) return;                                    // (uniform for the workgroup)
    const long hi = min(lo + EV_TILE, M);
    base[tid] = table[(long)blockIdx.x * 256 + tid];
#pragma unroll
    for (int w = 0; w < 4; ++w) wcnt[w][tid] = 0;
    __syncthreads();
    for (long c0 = lo; c0 < hi; c0 += 256) {
        const long i = c0 + tid;
        const bool valid = i < hi;
        u32x4 r = {0u, 0u, 0u, 0u};
        unsigned d = 0;
        if (valid) {
            r = src[i];
            d = (F::get(r, field, C) >> shift) & 255u;
        }
        // the lanes of this wave with the same digit: eight ballots
        unsigned long long peers = __ballot(valid);
#pragma unroll
        for (int bit = 0; bit < 8; ++bit) {
            const bool one = (d >> bit) & 1u;
            const unsigned long long m = __ballot(valid && one);
            peers &= one ? m : ~m;
        }
        const int rank = __popcll(peers & ((1ull << lane) - 1ull));
        if (valid && rank == 0) wcnt[wave][d] = __popcll(peers);
        __syncthreads();
        if (valid) {
            int pos = base[d] + rank;
#pragma unroll
            for (int w = 0; w < 4; ++w) pos += w < wave ? wcnt[w][d] : 0;
            if (pos >= 0 && (long)pos < M) dst[pos] = r;       // (always true when the table belongs to these records)
        }
        __syncthreads();
        {
            int add = 0;
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                add += wcnt[w][tid];
                wcnt[w][tid] = 0;
            }
            base[tid] += add;
        }
        __syncthreads();
    }
}

static inline int ev_bytes_for(unsigned long long max_value) {       // 8-bit digits needed for values 0 .. max_value
    int n = 1;
    while (n < 4 && (max_value >> (8 * n))) ++n;
    return n;
}
static inline long ev_tiles(long max_records) { return (max_records + EV_TILE - 1) / EV_TILE; }
static inline size_t ev_align(size_t v) { return (v + 255) / 256 * 256; }
