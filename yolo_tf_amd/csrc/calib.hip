// Calibration histograms of the int8 path (DESIGN.md section 15 "Calibration methods"): include/yolo2_hip.h yolo2_calib_histogram.  The
// specification is tests/calib_ref.py abs_histogram; the header states the bin rule.  Built with -ffp-contract=off: the bin index is one f32
// multiply and one truncation, everything behind it is integer, so the records are exact and the same whatever the order.
//
//   grid (CALIB_BLOCKS, njobs); a job's positions are cut into chunks of CALIB_CHUNK units and block x takes chunks x, x + CALIB_BLOCKS, ...
//
// A UNIT is one 16-byte load (8 bf16 / 4 f32) when the job allows it -- base 16-byte aligned and either dense (ld == c: the job is one flat
// run, its last total % V elements are counted by block 0) or c and ld both multiples of the vector (a concat member) -- else one element.
//   * counts: one u32 histogram per wave in LDS (4 x 2048 x 4 B = 32 KB).  Leaky activations put most values into the lowest bins, so the
//     hazard is same-address LDS atomics: four copies quarter them, and a wave whose 64 lanes agree adds 64 once.
//   * a workgroup flushes after EVERY chunk (non-zero bins, 64-bit global integer atomics) and zeroes its copies: a u32 counter never holds
//     more than one chunk's elements, CALIB_CHUNK * 8 = 65536 (+ 7 for the dense tail), far below 2^32, whatever the job's size.
//   * the non-finite and clamped counts stay in a u32 register per thread until the end: a thread sees at most
//     2^40 / (CALIB_BLOCKS * 256) = 2^24 elements of a job (rows * ld <= 2^40 is checked; a larger job is treated as empty).
#include "common.h"
#include <float.h>

#define CALIB_BLOCKS 256
#define CALIB_THREADS 256
#define CALIB_CHUNK 8192      // units per chunk: 32 per thread
#define CALIB_BATCH 4         // loads in flight per thread
static_assert(CALIB_CHUNK % (CALIB_THREADS * CALIB_BATCH) == 0, "a chunk is whole batches");
static_assert(sizeof(yolo2_calib_job) == 40, "descriptor layout");

// the tensors are global memory: loads through address space 1 are global_load (a generic pointer read from the job table would make them
// flat loads, which also count on the LDS counter the histogram's atomics wait on)
#define CALIB_GLOBAL(T, ptr) ((const __attribute__((address_space(1))) T *)(ptr))

template <int DTYPE, int V> __device__ __forceinline__ void calib_load(const void *base, long long p, float (&v)[V]) {
    if (DTYPE == YOLO2_F32) {
        if (V == 4) {
            const f32x4 q = *CALIB_GLOBAL(f32x4, (const float *)base + p);
#pragma unroll
            for (int k = 0; k < V; ++k) v[k] = q[k];
        } else {
            v[0] = *CALIB_GLOBAL(float, (const float *)base + p);
        }
    } else {
        if (V == 8) {
            const u32x4 q = *CALIB_GLOBAL(u32x4, (const unsigned short *)base + p);
#pragma unroll
            for (int k = 0; k < V; ++k) v[k] = __uint_as_float((k & 1) ? (q[k >> 1] & 0xffff0000u) : (q[k >> 1] << 16));
        } else {
            v[0] = __uint_as_float((unsigned)*CALIB_GLOBAL(unsigned short, (const unsigned short *)base + p) << 16);
        }
    }
}

// one element per lane; the whole wave calls this together (ok == false: the lane has no element)
__device__ __forceinline__ void calib_count(float x, bool ok, float limit, float inv_width, unsigned *cnt, unsigned &nonfinite, unsigned &clamped) {
    const float a = fabsf(x);
    int b = -1;
    if (ok) {
        if (a <= FLT_MAX) {
            const float t = a * inv_width;                       // one multiply, one rounding
            b = t >= (float)YOLO2_CALIB_BINS ? YOLO2_CALIB_BINS - 1 : (int)t;      // compare first: t may be +inf
            clamped += a > limit ? 1u : 0u;
        } else {
            ++nonfinite;                                         // inf or NaN: counted, in no bin
        }
    }
    const int b0 = __builtin_amdgcn_readfirstlane(b);
    if (__all(b == b0)) {                                        // a constant tensor, a dead layer: one add of 64
        if (b0 >= 0 && (threadIdx.x & 63) == 0) atomicAdd(cnt + b0, 64u);
    } else if (b >= 0) {
        atomicAdd(cnt + b, 1u);
    }
}

// units u0 .. uend-1 of the job; STRIDED: unit u sits at row u / cu, column u % cu of rows that are ldu units apart
template <int DTYPE, int V, bool STRIDED>
__device__ __forceinline__ void calib_chunk(const void *base, long long u0, long long uend, unsigned cu, long long ldu, float limit, float inv_width,
                                            unsigned *cnt, unsigned &nonfinite, unsigned &clamped) {
    const int tid = threadIdx.x;
    const long long r0 = STRIDED ? u0 / cu : 0;                  // (uniform: one 64-bit division per chunk)
    const unsigned c0 = STRIDED ? (unsigned)(u0 - r0 * cu) : 0u;
    for (int i = 0; i < CALIB_CHUNK / CALIB_THREADS; i += CALIB_BATCH) {
        float v[CALIB_BATCH][V];
        bool ok[CALIB_BATCH];
#pragma unroll
        for (int u = 0; u < CALIB_BATCH; ++u) {                  // the batch's loads first
            const unsigned o = (unsigned)(i + u) * CALIB_THREADS + tid;
            ok[u] = u0 + o < uend;
            long long p = u0 + o;
            if (STRIDED) {
                const unsigned col = c0 + o;                     // < 2^31 + CALIB_CHUNK
                p = (r0 + col / cu) * ldu + col % cu;
            }
            if (ok[u]) {
                calib_load<DTYPE, V>(base, p * V, v[u]);
            } else {
#pragma unroll
                for (int k = 0; k < V; ++k) v[u][k] = 0.f;
            }
        }
#pragma unroll
        for (int u = 0; u < CALIB_BATCH; ++u)
#pragma unroll
            for (int k = 0; k < V; ++k) calib_count(v[u][k], ok[u], limit, inv_width, cnt, nonfinite, clamped);
    }
}

__global__ __launch_bounds__(CALIB_THREADS) void calib_hist_kernel(const yolo2_calib_job *__restrict__ jobs, unsigned long long *__restrict__ out) {
    __shared__ unsigned cnt[4][YOLO2_CALIB_BINS];
    const yolo2_calib_job job = jobs[blockIdx.y];
    const int tid = threadIdx.x, wave = tid >> 6;
    // a descriptor that makes no sense owns no element (the Python host checks extents, slots and limits before it builds one)
    if (job.base == nullptr || job.rows <= 0 || job.c <= 0 || job.ld < job.c || job.slot < 0 || (job.dtype != YOLO2_F32 && job.dtype != YOLO2_BF16)) return;
    if (job.rows > (1LL << 40) / job.ld) return;
    if (!(job.limit > 0.f && job.limit <= FLT_MAX && job.inv_width > 0.f && job.inv_width <= FLT_MAX)) return;      // t = a * inv_width is then >= 0
    const bool f32 = job.dtype == YOLO2_F32;
    const int V = f32 ? 4 : 8;
    const bool dense = job.ld == job.c;
    const bool vec = ((uintptr_t)job.base & 15) == 0 && (dense || (job.c % V == 0 && job.ld % V == 0));
    const int U = vec ? V : 1;
    const long long total = job.rows * job.c;
    // dense: one flat row of `total` elements; otherwise rows of cu units, ldu units apart
    const long long nunits = dense ? total / U : job.rows * (job.c / U);
    const unsigned cu = dense ? 1u : (unsigned)(job.c / U);
    const long long ldu = job.ld / U;
    const int tail = dense ? (int)(total - nunits * U) : 0;     // < V elements behind the last whole vector
    const long long nchunks = (nunits + CALIB_CHUNK - 1) / CALIB_CHUNK;
    const bool has_tail = tail > 0 && blockIdx.x == 0;
    if ((long long)blockIdx.x >= nchunks && !has_tail) return;  // (block-uniform)
    for (int i = tid; i < 4 * YOLO2_CALIB_BINS; i += CALIB_THREADS) (&cnt[0][0])[i] = 0u;
    __syncthreads();
    unsigned long long *rec = out + (long long)job.slot * YOLO2_CALIB_WORDS;
    unsigned nonfinite = 0u, clamped = 0u;
    auto flush = [&]() {
        __syncthreads();
        for (int b = tid; b < YOLO2_CALIB_BINS; b += CALIB_THREADS) {
            const unsigned long long n = (unsigned long long)cnt[0][b] + cnt[1][b] + cnt[2][b] + cnt[3][b];
            if (n) {
                atomicAdd(rec + b, n);
                cnt[0][b] = cnt[1][b] = cnt[2][b] = cnt[3][b] = 0u;
            }
        }
        __syncthreads();
    };
    if (has_tail) {
        float v[1];
        const bool ok = tid < tail;
        v[0] = 0.f;
        if (ok) { if (f32) calib_load<YOLO2_F32, 1>(job.base, nunits * U + tid, v); else calib_load<YOLO2_BF16, 1>(job.base, nunits * U + tid, v); }
        calib_count(v[0], ok, job.limit, job.inv_width, cnt[wave], nonfinite, clamped);
        flush();
    }
    for (long long ch = blockIdx.x; ch < nchunks; ch += CALIB_BLOCKS) {
        const long long u0 = ch * CALIB_CHUNK;
        const long long uend = u0 + CALIB_CHUNK < nunits ? u0 + CALIB_CHUNK : nunits;
#define CALIB_GO(D, W) \
        do { if (dense) calib_chunk<D, W, false>(job.base, u0, uend, cu, ldu, job.limit, job.inv_width, cnt[wave], nonfinite, clamped); \
             else calib_chunk<D, W, true>(job.base, u0, uend, cu, ldu, job.limit, job.inv_width, cnt[wave], nonfinite, clamped); } while (0)
        if (f32) { if (vec) CALIB_GO(YOLO2_F32, 4); else CALIB_GO(YOLO2_F32, 1); }
        else { if (vec) CALIB_GO(YOLO2_BF16, 8); else CALIB_GO(YOLO2_BF16, 1); }
#undef CALIB_GO
        flush();
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        nonfinite += (unsigned)__shfl_xor((int)nonfinite, o, 64);
        clamped += (unsigned)__shfl_xor((int)clamped, o, 64);
    }
    if ((tid & 63) == 0) {
        if (nonfinite) atomicAdd(rec + YOLO2_CALIB_BINS, (unsigned long long)nonfinite);
        if (clamped) atomicAdd(rec + YOLO2_CALIB_BINS + 1, (unsigned long long)clamped);
    }
}

extern "C" int yolo2_calib_histogram(const yolo2_calib_job *jobs, int njobs, unsigned long long *out, void *stream) {
    Y2_CHECK_ARG(jobs && out && njobs > 0 && njobs <= 65535);
    Y2_CHECK_ARG(((uintptr_t)out & 7) == 0 && ((uintptr_t)jobs & 7) == 0);
    calib_hist_kernel<<<dim3(CALIB_BLOCKS, (unsigned)njobs), dim3(CALIB_THREADS), 0, (hipStream_t)stream>>>(jobs, out);
    Y2_CHECK_LAUNCH();
    return YOLO2_OK;
}
