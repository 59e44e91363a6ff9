// Gradient accumulation over micro-batches, the 1/K mean and weight decay in one streaming launch over the flat f32 arenas, gfx950.
// Built with -ffp-contract=off: every operation of an element is rounded once, in the order of the NumPy specification (tests/grad_combine_ref.py).
#include "common.h"

#define GC_THREADS 256
#define GC_CHUNK YOLO2_GRAD_COMBINE_CHUNK      // elements of one workgroup's chunk: four 16-byte accesses per thread and arena
#define GC_VECS (GC_CHUNK / 4 / GC_THREADS)
static_assert(GC_VECS * 4 * GC_THREADS == GC_CHUNK, "chunk = whole 16-byte accesses of every thread");

// mode FINAL, one element: the sum of the micro-gradients, its mean, the L2 term
__device__ __forceinline__ float gc_final_one(float g, float a, bool has_acc, float scale, bool dec, float decay, float w) {
    float s = g;
    if (has_acc) s = a + s;
    s = s * scale;
    if (dec) {
        const float t = decay * w;
        s = s + t;
    }
    return s;
}

// first range at or after r whose end lies behind element i (the ranges are sorted and disjoint: a walk forward), and whether it holds i
__device__ __forceinline__ bool gc_in_range(const long *__restrict__ ranges, int nr, int &r, long i) {
    while (r < nr && ranges[2 * r + 1] <= i) ++r;
    return r < nr && ranges[2 * r] <= i;
}

// Chunks are cut on 16-byte boundaries of g: `pre` = elements between the boundary at or below g and g, so that element i sits at virtual index i + pre and
// chunk c holds the virtual indices [c * GC_CHUNK, (c + 1) * GC_CHUNK).  `vec`: acc and w (where read) are aligned like g, 16-byte accesses are legal.
// A chunk that lies whole inside [0, n) and whole inside or whole outside the ranges takes 16-byte accesses only, all loads ahead of the arithmetic; every other
// chunk (the first and last of the arena, the ones a range begins or ends in, and all of them when vec == 0) takes the general path.
// HBM traffic per element: STORE 8 B, ADD 12 B, FINAL 8 B (+ 4 B with acc, + 4 B reading w where it decays, + 4 B writing w where it shrinks).
template <int MODE>
__global__ __launch_bounds__(GC_THREADS) void grad_combine_kernel(float *__restrict__ g, float *__restrict__ acc, float *__restrict__ w, long n, int pre, int vec,
                                                                  float scale, float decay, float shrink, const long *__restrict__ ranges, int nr, long nchunks) {
    const bool has_acc = MODE != YOLO2_GRAD_FINAL || acc != nullptr;
    const bool dec = MODE == YOLO2_GRAD_FINAL && nr > 0 && decay != 0.f;
    const bool shr = MODE == YOLO2_GRAD_FINAL && nr > 0 && shrink != 1.f;
    for (long c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const long first = c * GC_CHUNK - pre;                        // element of the chunk's virtual start (negative in chunk 0 when pre > 0)
        const long lo = first < 0 ? 0 : first;
        const long hi = first + GC_CHUNK < n ? first + GC_CHUNK : n;
        // the chunk's place among the ranges, once per workgroup: uniform binary search for the first range that ends behind lo
        int r0 = 0, cover = 0;                                        // cover: 0 no element in a range, 1 every element in ONE range, 2 mixed
        if (dec || shr) {
            int a = 0, b = nr;
            while (a < b) {
                const int m = (a + b) >> 1;
                if (ranges[2 * m + 1] <= lo) a = m + 1; else b = m;
            }
            r0 = a;
            if (r0 < nr && ranges[2 * r0] < hi) cover = (ranges[2 * r0] <= lo && ranges[2 * r0 + 1] >= hi) ? 1 : 2;
        }
        if (vec && first >= 0 && first + GC_CHUNK <= n && cover != 2) {
            // (first + pre is a multiple of GC_CHUNK and g - pre lies on a 16-byte boundary: g + first does, and with vec so do acc + first and w + first)
            const int v = threadIdx.x;
            const bool in = cover == 1;
            f32x4 *g4 = reinterpret_cast<f32x4 *>(g + first);
            f32x4 *a4 = has_acc ? reinterpret_cast<f32x4 *>(acc + first) : nullptr;
            f32x4 *w4 = in ? reinterpret_cast<f32x4 *>(w + first) : nullptr;
            f32x4 gv[GC_VECS], av[GC_VECS], wv[GC_VECS];
#pragma unroll
            for (int j = 0; j < GC_VECS; ++j) gv[j] = g4[v + j * GC_THREADS];
            if (MODE != YOLO2_GRAD_STORE && has_acc) {
#pragma unroll
                for (int j = 0; j < GC_VECS; ++j) av[j] = a4[v + j * GC_THREADS];
            }
            if (in) {
#pragma unroll
                for (int j = 0; j < GC_VECS; ++j) wv[j] = w4[v + j * GC_THREADS];
            }
#pragma unroll
            for (int j = 0; j < GC_VECS; ++j) {
                if (MODE == YOLO2_GRAD_STORE) {
                    a4[v + j * GC_THREADS] = gv[j];
                } else if (MODE == YOLO2_GRAD_ADD) {
                    f32x4 s;
#pragma unroll
                    for (int k = 0; k < 4; ++k) s[k] = av[j][k] + gv[j][k];
                    a4[v + j * GC_THREADS] = s;
                } else {
                    f32x4 s;
#pragma unroll
                    for (int k = 0; k < 4; ++k) s[k] = gc_final_one(gv[j][k], has_acc ? av[j][k] : 0.f, has_acc, scale, in && dec, decay, in ? wv[j][k] : 0.f);
                    g4[v + j * GC_THREADS] = s;
                    if (in && shr) {
                        f32x4 t;
#pragma unroll
                        for (int k = 0; k < 4; ++k) t[k] = wv[j][k] * shrink;
                        w4[v + j * GC_THREADS] = t;
                    }
                }
            }
            continue;
        }
        // general path: a thread's elements ascend with j, so its walk over the ranges only moves forward from r0
        int r = r0;
#pragma unroll
        for (int j = 0; j < GC_VECS; ++j) {
            const long i0 = first + 4L * (threadIdx.x + j * GC_THREADS);
            if (i0 >= hi || i0 + 4 <= lo) continue;
            if (vec && i0 >= lo && i0 + 4 <= hi) {                    // a whole 16-byte group inside the arena: vector g and acc, w by element
                f32x4 gv = *reinterpret_cast<f32x4 *>(g + i0), s;
                if (MODE == YOLO2_GRAD_STORE) {
                    s = gv;
                } else {
                    f32x4 av = {0.f, 0.f, 0.f, 0.f};
                    if (has_acc) av = *reinterpret_cast<f32x4 *>(acc + i0);
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        if (MODE == YOLO2_GRAD_ADD) {
                            s[k] = av[k] + gv[k];
                        } else {
                            const bool in = cover != 0 && gc_in_range(ranges, nr, r, i0 + k);
                            const float wk = in ? w[i0 + k] : 0.f;
                            s[k] = gc_final_one(gv[k], av[k], has_acc, scale, in && dec, decay, wk);
                            if (in && shr) w[i0 + k] = wk * shrink;
                        }
                    }
                }
                *reinterpret_cast<f32x4 *>((MODE == YOLO2_GRAD_FINAL ? g : acc) + i0) = s;
                continue;
            }
            for (int k = 0; k < 4; ++k) {                             // scalar head / tail (and every element of arenas that are not aligned alike)
                const long i = i0 + k;
                if (i < lo || i >= hi) continue;
                if (MODE == YOLO2_GRAD_STORE) {
                    acc[i] = g[i];
                } else if (MODE == YOLO2_GRAD_ADD) {
                    acc[i] = acc[i] + g[i];
                } else {
                    const bool in = cover != 0 && gc_in_range(ranges, nr, r, i);
                    const float wk = in ? w[i] : 0.f;
                    g[i] = gc_final_one(g[i], has_acc ? acc[i] : 0.f, has_acc, scale, in && dec, decay, wk);
                    if (in && shr) w[i] = wk * shrink;
                }
            }
        }
    }
}

extern "C" int yolo2_grad_combine(float *g, float *acc, float *w, long n, int mode, float scale, float decay, float shrink,
                                  const long *ranges_device, int n_ranges, void *stream) {
    Y2_CHECK_ARG(n >= 0 && n_ranges >= 0);
    Y2_CHECK_ARG(mode == YOLO2_GRAD_STORE || mode == YOLO2_GRAD_ADD || mode == YOLO2_GRAD_FINAL);
    Y2_CHECK_ARG(mode == YOLO2_GRAD_FINAL || acc != nullptr);
    const bool decays = mode == YOLO2_GRAD_FINAL && n_ranges > 0 && (decay != 0.f || shrink != 1.f);
    Y2_CHECK_ARG(!decays || (ranges_device != nullptr && w != nullptr));
    if (n == 0) return YOLO2_OK;
    Y2_CHECK_ARG(g != nullptr);
    Y2_CHECK_ARG((((uintptr_t)g) | ((uintptr_t)acc) | ((uintptr_t)w)) % sizeof(float) == 0);
    if (!decays) n_ranges = 0;                                         // (the kernel then never reads w or the table)
    const unsigned mis = (unsigned)((uintptr_t)g & 15);
    const int pre = (int)(mis / sizeof(float));
    const bool reads_acc = mode != YOLO2_GRAD_FINAL || acc != nullptr;
    const int vec = (!reads_acc || ((uintptr_t)acc & 15) == mis) && (!decays || ((uintptr_t)w & 15) == mis);
    const long nchunks = (n + pre + GC_CHUNK - 1) / GC_CHUNK;
    // memory-bound: eight 256-thread workgroups per CU, the chunk-stride loop takes the rest
    long blocks = nchunks;
    const long cap = 8L * y2_device_cus();
    if (blocks > cap) blocks = cap;
    hipStream_t st = (hipStream_t)stream;
    if (mode == YOLO2_GRAD_STORE)
        grad_combine_kernel<YOLO2_GRAD_STORE><<<(int)blocks, GC_THREADS, 0, st>>>(g, acc, w, n, pre, vec, scale, decay, shrink, ranges_device, n_ranges, nchunks);
    else if (mode == YOLO2_GRAD_ADD)
        grad_combine_kernel<YOLO2_GRAD_ADD><<<(int)blocks, GC_THREADS, 0, st>>>(g, acc, w, n, pre, vec, scale, decay, shrink, ranges_device, n_ranges, nchunks);
    else
        grad_combine_kernel<YOLO2_GRAD_FINAL><<<(int)blocks, GC_THREADS, 0, st>>>(g, acc, w, n, pre, vec, scale, decay, shrink, ranges_device, n_ranges, nchunks);
    Y2_CHECK_LAUNCH();
    return YOLO2_OK;
}
