// Image summaries (tf.summary.image's NormalizeFloatImage plus the reference's channel sum) of many device tensors in one call:
// include/yolo2_hip.h yolo2_image_summary.  The specification is tests/image_summary_ref.py; DESIGN.md "Image summaries" has the design.
//
//   memset(ws header)  ->  img_reduce_kernel (one workgroup per work item)  ->  img_scale_kernel (one thread per job)  ->  img_map_kernel (as the first)
//
// A JOB is one image: rows = H*W pixels of c values every ld elements.  One THREAD owns a pixel, so a pixel's channel sum is one thread's own
// sequential chain and its order is the specification's by construction; a work item is Y2_IMG_THREADS * k consecutive pixels with k chosen
// from c alone (about 16K elements per item), a split that depends on nothing but the job's own shape.
//   * reduce: the f32 value(s) of every pixel -- for c outside {1, 3, 4} the channel sum, stored into the workspace so that the map pass reads 4
//     bytes a pixel instead of c elements and the f64 chain runs once -- and the min / max over the finite pixels as unsigned keys that order
//     like the floats: wave butterfly, the four waves through LDS, one integer atomicMax pair per work item.  Integers: exact in any order.
//   * scale: keys -> image_min, image_max, scale (an IEEE f32 division), offset; the job's record.
//   * map: byte = uint8(trunc(x * scale + offset)), multiply and add rounded separately (this unit is built with -ffp-contract=off); a pixel with
//     a non-finite value gets the bad colour.  Plain byte stores.
#include "common.h"
#include <math.h>

#define Y2_IMG_THREADS 256
#define Y2_IMG_HEADER_WORDS 8      // per job in ws: max key, ~min key, non-finite pixels, -, scale, offset, -, -
static_assert(YOLO2_IMAGE_RECORD_BYTES == 16, "record: min, max (f32), non-finite pixels (u32), scale (f32)");
static_assert(YOLO2_IMAGE_GROUP == 8, "one 16-byte load of bf16 is one group of the channel sum");

__host__ __device__ static inline int y2_img_depth(int c) { return (c == 1 || c == 3 || c == 4) ? c : 1; }
// pixels of one work item: 256 threads x k pixels each, k = 64 / c clamped to 1 .. 16
__host__ __device__ static inline int y2_img_item_pixels(int c) {
    int k = c > 0 ? 64 / c : 1;
    k = k < 1 ? 1 : (k > 16 ? 16 : k);
    return Y2_IMG_THREADS * k;
}
// a descriptor that makes no sense owns no pixel (the Python host checks extents against the tensors before it builds one)
__host__ __device__ static inline long long y2_img_rows(long long rows, int c, int ld, int dtype) {
    if (rows <= 0 || rows > 0x7fffffffLL || c <= 0 || ld < c || (dtype != YOLO2_F32 && dtype != YOLO2_BF16)) return 0;
    return rows;
}
__host__ __device__ static inline int y2_img_items(long long rows, int c, int ld, int dtype) {
    const long long r = y2_img_rows(rows, c, ld, dtype);
    const int ppi = y2_img_item_pixels(c);
    return (int)((r + ppi - 1) / ppi);
}
// ... and one whose output or sums would leave the buffers of the call owns none either
__device__ __forceinline__ long long y2_img_job_rows(const yolo2_image_job &job, int njobs, unsigned long long out_bytes, unsigned long long sum_floats) {
    const long long r = y2_img_rows(job.rows, job.c, job.ld, job.dtype);
    if (r == 0) return 0;
    const unsigned long long bytes = (unsigned long long)r * y2_img_depth(job.c);
    if (job.out_offset < (long long)njobs * YOLO2_IMAGE_RECORD_BYTES || (unsigned long long)job.out_offset > out_bytes || bytes > out_bytes - (unsigned long long)job.out_offset) return 0;
    if (y2_img_depth(job.c) != job.c && (job.sum_offset < 0 || (unsigned long long)job.sum_offset > sum_floats || (unsigned long long)r > sum_floats - (unsigned long long)job.sum_offset)) return 0;
    return r;
}

template <int DTYPE> __device__ __forceinline__ float y2_img_load(const void *base, long long p) {
    if (DTYPE == YOLO2_F32) return ((const float *)base)[p];
    return __uint_as_float((unsigned)((const unsigned short *)base)[p] << 16);
}
// the eight values of one channel group starting at element p; VEC: 16-byte loads (p is then a multiple of 8 elements from an aligned base)
template <int DTYPE, bool VEC> __device__ __forceinline__ void y2_img_load8(const void *base, long long p, float *v) {
    if (VEC && DTYPE == YOLO2_BF16) {
        const u32x4 w = *(const u32x4 *)((const unsigned short *)base + p);
#pragma unroll
        for (int i = 0; i < 4; ++i) { v[2 * i] = __uint_as_float(w[i] << 16); v[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u); }
    } else if (VEC) {
        const f32x4 a = *(const f32x4 *)((const float *)base + p), b = *(const f32x4 *)((const float *)base + p + 4);
#pragma unroll
        for (int i = 0; i < 4; ++i) { v[i] = a[i]; v[4 + i] = b[i]; }
    } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = y2_img_load<DTYPE>(base, p + i);
    }
}
__device__ __forceinline__ double y2_img_chain8(const float *v) {
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < 8; ++i) s += (double)v[i];
    return s;
}
// The specification's channel sum of the pixel at element p: f64, sequential from +0.0 inside every group of 8 consecutive channels (the last
// group may be short), the group partials added to a total that starts at +0.0 in ascending order, one rounding to f32.  Four groups are loaded
// and chained side by side -- independent chains, the same additions.
template <int DTYPE, bool VEC> __device__ __forceinline__ float y2_img_channel_sum(const void *base, long long p, int c) {
    double total = 0.0;
    const int ng = c >> 3;
    int g = 0;
    for (; g + 4 <= ng; g += 4) {
        float v[4][8];
#pragma unroll
        for (int u = 0; u < 4; ++u) y2_img_load8<DTYPE, VEC>(base, p + 8 * (g + u), v[u]);
        double part[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) part[u] = y2_img_chain8(v[u]);
#pragma unroll
        for (int u = 0; u < 4; ++u) total += part[u];
    }
    for (; g < ng; ++g) {
        float v[8];
        y2_img_load8<DTYPE, VEC>(base, p + 8 * g, v);
        total += y2_img_chain8(v);
    }
    if (c & 7) {                                                // lanes c .. ld-1 are never read
        double part = 0.0;
        for (int j = ng * 8; j < c; ++j) part += (double)y2_img_load<DTYPE>(base, p + j);
        total += part;
    }
    return (float)total;
}

__device__ __forceinline__ bool y2_img_finite(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }
// unsigned keys in the order of the floats (-0 below +0); every finite value's key lies strictly between 0x00800000 and 0xff800000
__device__ __forceinline__ unsigned y2_img_key(float x) {
    const unsigned b = __float_as_uint(x);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float y2_img_unkey(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// the job of work item `item`: the last one whose first_item is <= item (jobs without pixels own no item and are never found)
__device__ __forceinline__ int y2_img_find(const yolo2_image_job *jobs, int njobs, int item) {
    int lo = 0, hi = njobs - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (jobs[mid].first_item <= item) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// this thread's pixel values (n = depth of them in v) -> whether all are finite
template <int DTYPE> __device__ __forceinline__ bool y2_img_pixel(const yolo2_image_job &job, bool vec, const float *sums, long long px, bool map, float *v, int depth) {
    if (depth != job.c) {
        if (map) {
            v[0] = sums[job.sum_offset + px];
        } else {
            const long long p = px * (long long)job.ld;
            v[0] = vec ? y2_img_channel_sum<DTYPE, true>(job.base, p, job.c) : y2_img_channel_sum<DTYPE, false>(job.base, p, job.c);
        }
        return y2_img_finite(v[0]);
    }
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 4; ++j) {                               // (unrolled with a guard: v stays in registers)
        if (j < depth) {
            v[j] = y2_img_load<DTYPE>(job.base, px * (long long)job.ld + j);
            ok = ok && y2_img_finite(v[j]);
        }
    }
    return ok;
}

template <int DTYPE>
__device__ __forceinline__ void y2_img_reduce_item(const yolo2_image_job &job, long long rows, int slot, float *sums, unsigned *hdr, unsigned (*red)[3]) {
    const int tid = threadIdx.x, wave = tid >> 6, depth = y2_img_depth(job.c), ppi = y2_img_item_pixels(job.c);
    const bool vec = ((uintptr_t)job.base & 15) == 0 && job.ld % (DTYPE == YOLO2_BF16 ? 8 : 4) == 0;
    const long long p0 = (long long)slot * ppi, pend = p0 + ppi < rows ? p0 + ppi : rows;
    unsigned kmax = 0u, kmin_inv = 0u, bad = 0u;                // 0 = none yet: below every finite value's key (and its complement)
    for (long long px = p0 + tid; px < pend; px += Y2_IMG_THREADS) {
        float v[4];
        const bool ok = y2_img_pixel<DTYPE>(job, vec, sums, px, false, v, depth);
        if (depth != job.c) sums[job.sum_offset + px] = v[0];
        if (ok) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (j < depth) {
                    const unsigned k = y2_img_key(v[j]);
                    kmax = k > kmax ? k : kmax;
                    kmin_inv = ~k > kmin_inv ? ~k : kmin_inv;
                }
            }
        } else {
            bad += 1u;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned a = __shfl_xor(kmax, o, 64), b = __shfl_xor(kmin_inv, o, 64);
        kmax = a > kmax ? a : kmax;
        kmin_inv = b > kmin_inv ? b : kmin_inv;
        bad += __shfl_xor(bad, o, 64);
    }
    if ((tid & 63) == 0) { red[wave][0] = kmax; red[wave][1] = kmin_inv; red[wave][2] = bad; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < Y2_IMG_THREADS / 64; ++w) {
            kmax = red[w][0] > kmax ? red[w][0] : kmax;
            kmin_inv = red[w][1] > kmin_inv ? red[w][1] : kmin_inv;
            bad += red[w][2];
        }
        if (kmax) { atomicMax(hdr + 0, kmax); atomicMax(hdr + 1, kmin_inv); }      // (integers: any order gives the same words)
        if (bad) atomicAdd(hdr + 2, bad);
    }
}

__global__ __launch_bounds__(Y2_IMG_THREADS) void img_reduce_kernel(const yolo2_image_job *__restrict__ jobs, int njobs, unsigned long long out_bytes,
                                                                     unsigned *__restrict__ ws, unsigned long long sum_floats) {
    __shared__ unsigned red[Y2_IMG_THREADS / 64][3];
    const int j = y2_img_find(jobs, njobs, (int)blockIdx.x);
    const yolo2_image_job job = jobs[j];
    const long long rows = y2_img_job_rows(job, njobs, out_bytes, sum_floats);
    const int slot = (int)blockIdx.x - job.first_item;
    if (slot < 0 || slot >= y2_img_items(rows, job.c, job.ld, job.dtype)) return;      // (block-uniform; a table whose item counts do not match its shapes)
    float *sums = (float *)(ws + (long long)njobs * Y2_IMG_HEADER_WORDS);
    unsigned *hdr = ws + (long long)j * Y2_IMG_HEADER_WORDS;
    if (job.dtype == YOLO2_F32) y2_img_reduce_item<YOLO2_F32>(job, rows, slot, sums, hdr, red);
    else y2_img_reduce_item<YOLO2_BF16>(job, rows, slot, sums, hdr, red);
}

// one thread per job: NormalizeFloatImage's scale and offset from the min / max of the finite pixels
__global__ __launch_bounds__(Y2_IMG_THREADS) void img_scale_kernel(int njobs, unsigned *__restrict__ ws, unsigned char *__restrict__ out) {
    const int j = blockIdx.x * Y2_IMG_THREADS + threadIdx.x;
    if (j >= njobs) return;
    unsigned *hdr = ws + (long long)j * Y2_IMG_HEADER_WORDS;
    const bool any = hdr[0] != 0u;
    const float mn = any ? y2_img_unkey(~hdr[1]) : INFINITY, mx = any ? y2_img_unkey(hdr[0]) : -INFINITY;
    const float zero = 1e-6f;
    float scale, offset;
    if (mn < 0.f) {
        const float m = fmaxf(fabsf(mn), fabsf(mx));
        scale = m < zero ? 0.f : 127.f / m;
        offset = 128.f;
    } else {
        scale = mx < zero ? 0.f : 255.f / mx;
        offset = 0.f;
    }
    hdr[4] = __float_as_uint(scale);
    hdr[5] = __float_as_uint(offset);
    unsigned *rec = (unsigned *)(out + (long long)j * YOLO2_IMAGE_RECORD_BYTES);
    rec[0] = __float_as_uint(mn);
    rec[1] = __float_as_uint(mx);
    rec[2] = hdr[2];
    rec[3] = __float_as_uint(scale);
}

template <int DTYPE>
__device__ __forceinline__ void y2_img_map_item(const yolo2_image_job &job, long long rows, int slot, const float *sums, float scale, float offset, unsigned char *out) {
    const int tid = threadIdx.x, depth = y2_img_depth(job.c), ppi = y2_img_item_pixels(job.c);
    const long long p0 = (long long)slot * ppi, pend = p0 + ppi < rows ? p0 + ppi : rows;
    unsigned char *o = out + job.out_offset;
    for (long long px = p0 + tid; px < pend; px += Y2_IMG_THREADS) {
        float v[4];
        const bool ok = y2_img_pixel<DTYPE>(job, false, sums, px, true, v, depth);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (j < depth) {
                const float y = v[j] * scale + offset;          // two roundings: contraction is off for this unit
                o[px * depth + j] = ok ? (unsigned char)(int)y : (unsigned char)((j == 0 || j == 3) ? 255 : 0);      // bad colour (255, 0, 0, 255)
            }
        }
    }
}

__global__ __launch_bounds__(Y2_IMG_THREADS) void img_map_kernel(const yolo2_image_job *__restrict__ jobs, int njobs, unsigned char *__restrict__ out,
                                                                  unsigned long long out_bytes, const unsigned *__restrict__ ws, unsigned long long sum_floats) {
    const int j = y2_img_find(jobs, njobs, (int)blockIdx.x);
    const yolo2_image_job job = jobs[j];
    const long long rows = y2_img_job_rows(job, njobs, out_bytes, sum_floats);
    const int slot = (int)blockIdx.x - job.first_item;
    if (slot < 0 || slot >= y2_img_items(rows, job.c, job.ld, job.dtype)) return;
    const float *sums = (const float *)(ws + (long long)njobs * Y2_IMG_HEADER_WORDS);
    const unsigned *hdr = ws + (long long)j * Y2_IMG_HEADER_WORDS;
    const float scale = __uint_as_float(hdr[4]), offset = __uint_as_float(hdr[5]);
    if (job.dtype == YOLO2_F32) y2_img_map_item<YOLO2_F32>(job, rows, slot, sums, scale, offset, out);
    else y2_img_map_item<YOLO2_BF16>(job, rows, slot, sums, scale, offset, out);
}

static inline size_t y2_img_count(long long n) { return n > 0 ? (size_t)n : 0; }
extern "C" size_t yolo2_image_summary_workspace_bytes(int njobs, long long sum_pixels) { return y2_img_count(njobs) * Y2_IMG_HEADER_WORDS * 4 + y2_img_count(sum_pixels) * 4; }
extern "C" size_t yolo2_image_summary_result_bytes(int njobs, long long image_bytes) { return y2_img_count(njobs) * YOLO2_IMAGE_RECORD_BYTES + y2_img_count(image_bytes); }
extern "C" int yolo2_image_summary_items(long long rows, int c, int ld, int dtype) { return y2_img_items(rows, c, ld, dtype); }
extern "C" int yolo2_image_summary_depth(int c) { return c > 0 ? y2_img_depth(c) : 0; }

extern "C" int yolo2_image_summary(const yolo2_image_job *jobs, int njobs, int items, void *out, size_t out_bytes, void *ws, size_t ws_bytes, void *stream) {
    static_assert(sizeof(yolo2_image_job) == 48, "descriptor layout");
    Y2_CHECK_ARG(jobs && out && ws && njobs > 0 && items >= 0);
    Y2_CHECK_ARG(out_bytes >= yolo2_image_summary_result_bytes(njobs, 0) && ws_bytes >= yolo2_image_summary_workspace_bytes(njobs, 0));
    Y2_CHECK_ARG(((uintptr_t)out & 3) == 0 && ((uintptr_t)ws & 3) == 0 && ((uintptr_t)jobs & 7) == 0);
    hipStream_t st = (hipStream_t)stream;
    const size_t header = (size_t)njobs * Y2_IMG_HEADER_WORDS * 4;
    const unsigned long long sum_floats = (ws_bytes - header) / 4;
    if (hipMemsetAsync(ws, 0, header, st) != hipSuccess) { yolo2_set_error("yolo2_image_summary: memset failed"); return YOLO2_E_LAUNCH; }
    if (items > 0) img_reduce_kernel<<<items, Y2_IMG_THREADS, 0, st>>>(jobs, njobs, (unsigned long long)out_bytes, (unsigned *)ws, sum_floats);
    img_scale_kernel<<<(njobs + Y2_IMG_THREADS - 1) / Y2_IMG_THREADS, Y2_IMG_THREADS, 0, st>>>(njobs, (unsigned *)ws, (unsigned char *)out);
    if (items > 0) img_map_kernel<<<items, Y2_IMG_THREADS, 0, st>>>(jobs, njobs, (unsigned char *)out, (unsigned long long)out_bytes, (const unsigned *)ws, sum_floats);
    Y2_CHECK_LAUNCH();
    return YOLO2_OK;
}
