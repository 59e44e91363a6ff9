// Histogram summaries (tf.summary.histogram's buckets and statistics) of many device tensors in one call: include/yolo2_hip.h
// yolo2_histogram.  The specification is tests/summary_ref.py; DESIGN.md "Histogram summaries" has the design and what bounds it.
//
//   memset(out)  ->  hist_bin_kernel (one workgroup per work item)  ->  hist_finalize_kernel (one workgroup per job)
//
// A JOB is one tensor: rows x c values with row stride ld.  Its element positions 0 .. extent-1 (extent = (rows-1)*ld + c; lanes c..ld-1 of
// a row are skipped) are cut into chunks of Y2_HIST_CHUNK; the job owns nslots = min(chunks, Y2_HIST_SLOTS) work items, and item s bins
// chunks s, s + nslots, ... -- a static assignment that depends on nothing but the job's own shape.
//   * counts are integers: per-wave u32 sub-histograms in LDS (a weight tensor lands in ~50 buckets: four copies quarter the same-address
//     traffic, a wave whose 64 lanes agree adds once), flushed with 64-bit global integer atomics -- exact, and the same whatever the order.
//   * sum and sum_squares are f64 chains with ONE writer each: thread (fixed stride) -> wave butterfly -> the four waves in order -> one stored
//     partial per work item -> the finalize pass adds a job's partials in slot order.  No float atomic anywhere, so the output bytes depend on
//     the job alone: not on the other jobs of the call, their order, or what runs beside it.
//   * the bucket is upper_bound on the f64 limits: an estimate from log2 of the magnitude, then corrected against the table in LDS until the two
//     neighbouring limits bracket the value -- the table decides, the estimate only saves the search.
#include "common.h"
#include "hist_limits.h"
#include <float.h>

#define Y2_HIST_CHUNK 16384
#define Y2_HIST_SLOTS 512
#define Y2_HIST_THREADS 256
#define Y2_HIST_BATCH 8
static_assert(YOLO2_HIST_BUCKETS == 2 * Y2_HIST_POS + 2, "limits: -pos reversed, 0, pos, DBL_MAX");
static_assert(Y2_HIST_CHUNK % (Y2_HIST_THREADS * Y2_HIST_BATCH) == 0, "a chunk is whole batches");

__device__ const double y2_hist_pos[Y2_HIST_POS] = {Y2_HIST_POS_LIST};

struct Y2HistPartial {
    double mn, mx, sum, sq;
    unsigned long long num, nonfinite;
};

// a descriptor that makes no sense owns no element (the Python host checks extents against the tensors before it builds one)
__host__ __device__ static inline long long y2_hist_extent(long long rows, int c, int ld, int dtype) {
    if (rows <= 0 || c <= 0 || ld < c || (dtype != YOLO2_F32 && dtype != YOLO2_BF16)) return 0;
    if (rows > (1LL << 40) / ld) return 0;
    return (rows - 1) * (long long)ld + c;
}
__host__ __device__ static inline long long y2_hist_chunks(long long extent) { return (extent + Y2_HIST_CHUNK - 1) / Y2_HIST_CHUNK; }
__host__ __device__ static inline int y2_hist_slots(long long extent) {
    const long long ch = y2_hist_chunks(extent);
    return ch < Y2_HIST_SLOTS ? (int)ch : Y2_HIST_SLOTS;
}

// upper_bound(limits, x) for finite x.  k = how many positive limits are <= |x| (kl: < |x|); limits = {-pos[773] .. -pos[0], 0, pos[0] .. pos[773], DBL_MAX}.
__device__ __forceinline__ int y2_hist_bucket(float x, const double *pos) {
    const float af = fabsf(x);
    if (af == 0.f) return Y2_HIST_POS + 1;                      // +0 and -0: above the limit 0.0
    const double a = (double)af;
    // pos[i] = 1e-12 * 1.1^i up to rounding: i ~ (log2|x| - log2 1e-12) / log2 1.1
    const float e = fminf(fmaxf((__log2f(af) + 39.8631371f) * 7.27254090f, -1.f), (float)Y2_HIST_POS);
    int k = min(max((int)floorf(e) + 1, 0), Y2_HIST_POS);
    while (k > 0 && pos[k - 1] > a) --k;
    while (k < Y2_HIST_POS && pos[k] <= a) ++k;
    if (x > 0.f) return Y2_HIST_POS + 1 + k;
    const int kl = (k > 0 && pos[k - 1] == a) ? k - 1 : k;      // a value equal to a limit goes to the bucket above: -pos[i] itself counts as <= x
    return Y2_HIST_POS - kl;
}

template <int DTYPE> __device__ __forceinline__ float y2_hist_load(const void *base, long long p) {
    if (DTYPE == YOLO2_F32) return ((const float *)base)[p];
    return __uint_as_float((unsigned)((const unsigned short *)base)[p] << 16);
}

struct Y2HistAcc {
    double mn, mx, sum, sq;
    unsigned long long num, nonfinite;
};

template <int DTYPE, bool STRIDED>
__device__ __forceinline__ void y2_hist_chunk(const void *base, long long p0, long long pend, int c, int ld, const double *pos, unsigned *cnt, Y2HistAcc &acc) {
    const int tid = threadIdx.x;
    const unsigned col0 = STRIDED ? (unsigned)(p0 % ld) : 0u;      // (uniform: one 64-bit remainder per chunk)
    for (int i = 0; i < Y2_HIST_CHUNK / Y2_HIST_THREADS; i += Y2_HIST_BATCH) {
        float v[Y2_HIST_BATCH];
        bool ok[Y2_HIST_BATCH];
#pragma unroll
        for (int u = 0; u < Y2_HIST_BATCH; ++u) {               // the batch's loads first: eight in flight per lane
            const unsigned o = (unsigned)(i + u) * Y2_HIST_THREADS + tid;
            const long long p = p0 + o;
            ok[u] = p < pend;
            if (STRIDED) ok[u] = ok[u] && (col0 + o) % (unsigned)ld < (unsigned)c;      // padding lanes never reach the result
            v[u] = ok[u] ? y2_hist_load<DTYPE>(base, p) : 0.f;
        }
#pragma unroll
        for (int u = 0; u < Y2_HIST_BATCH; ++u) {
            const float x = v[u];
            const bool finite = (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u;
            int b = -1;
            if (ok[u] && finite) {
                b = y2_hist_bucket(x, pos);
                const double d = (double)x;
                acc.sum += d;
                acc.sq += d * d;
                acc.mn = d < acc.mn ? d : acc.mn;
                acc.mx = d > acc.mx ? d : acc.mx;
                acc.num += 1;
            } else if (ok[u]) {
                acc.nonfinite += 1;
            }
            // all 64 lanes in one bucket (a constant tensor, a dead layer): one add of 64 instead of a 64-way same-address serialisation
            const int b0 = __builtin_amdgcn_readfirstlane(b);
            if (__all(b == b0)) {
                if (b0 >= 0 && (tid & 63) == 0) atomicAdd(cnt + b0, 64u);
            } else if (b >= 0) {
                atomicAdd(cnt + b, 1u);
            }
        }
    }
}

__global__ __launch_bounds__(Y2_HIST_THREADS) void hist_bin_kernel(const yolo2_hist_job *__restrict__ jobs, int njobs, unsigned long long *__restrict__ out,
                                                                    Y2HistPartial *__restrict__ ws) {
    __shared__ double pos[Y2_HIST_POS];
    __shared__ unsigned cnt[4][YOLO2_HIST_BUCKETS];
    __shared__ double red[4][4];
    __shared__ unsigned long long nred[2];
    const int tid = threadIdx.x, wave = tid >> 6;
    for (int i = tid; i < Y2_HIST_POS; i += Y2_HIST_THREADS) pos[i] = y2_hist_pos[i];
    for (int i = tid; i < 4 * YOLO2_HIST_BUCKETS; i += Y2_HIST_THREADS) (&cnt[0][0])[i] = 0u;
    if (tid < 2) nred[tid] = 0ull;
    // the job of this work item: the last one whose first_item is <= blockIdx.x (jobs without elements own no item and are never found)
    int lo = 0, hi = njobs - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (jobs[mid].first_item <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
    }
    const yolo2_hist_job job = jobs[lo];
    const int slot = (int)blockIdx.x - job.first_item;
    const long long extent = y2_hist_extent(job.rows, job.c, job.ld, job.dtype);
    const long long nchunks = y2_hist_chunks(extent);
    const int nslots = y2_hist_slots(extent);
    if (slot < 0 || slot >= nslots) return;                     // (block-uniform; a table whose item counts do not match its shapes)
    __syncthreads();
    Y2HistAcc acc = {DBL_MAX, -DBL_MAX, 0.0, 0.0, 0ull, 0ull};
    const bool strided = job.ld != job.c;
    for (long long ch = slot; ch < nchunks; ch += nslots) {
        const long long p0 = ch * Y2_HIST_CHUNK;
        const long long pend = p0 + Y2_HIST_CHUNK < extent ? p0 + Y2_HIST_CHUNK : extent;
        if (job.dtype == YOLO2_F32) {
            if (strided) y2_hist_chunk<YOLO2_F32, true>(job.base, p0, pend, job.c, job.ld, pos, cnt[wave], acc);
            else y2_hist_chunk<YOLO2_F32, false>(job.base, p0, pend, job.c, job.ld, pos, cnt[wave], acc);
        } else {
            if (strided) y2_hist_chunk<YOLO2_BF16, true>(job.base, p0, pend, job.c, job.ld, pos, cnt[wave], acc);
            else y2_hist_chunk<YOLO2_BF16, false>(job.base, p0, pend, job.c, job.ld, pos, cnt[wave], acc);
        }
    }
    // float partials: fixed butterfly inside the wave, the four waves in order, one store
    const double sum = wave_sum_d(acc.sum), sq = wave_sum_d(acc.sq);
    double mn = acc.mn, mx = acc.mx;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double m2 = __shfl_xor(mn, o, 64), x2 = __shfl_xor(mx, o, 64);
        mn = m2 < mn ? m2 : mn;
        mx = x2 > mx ? x2 : mx;
    }
    if ((tid & 63) == 0) { red[wave][0] = mn; red[wave][1] = mx; red[wave][2] = sum; red[wave][3] = sq; }
    if (acc.num) atomicAdd(&nred[0], acc.num);                  // (integers: any order)
    if (acc.nonfinite) atomicAdd(&nred[1], acc.nonfinite);
    __syncthreads();
    if (tid == 0) {
        Y2HistPartial p;
        p.mn = red[0][0]; p.mx = red[0][1];
        for (int w = 1; w < 4; ++w) { p.mn = red[w][0] < p.mn ? red[w][0] : p.mn; p.mx = red[w][1] > p.mx ? red[w][1] : p.mx; }
        p.sum = ((red[0][2] + red[1][2]) + red[2][2]) + red[3][2];
        p.sq = ((red[0][3] + red[1][3]) + red[2][3]) + red[3][3];
        p.num = nred[0]; p.nonfinite = nred[1];
        ws[(long long)lo * Y2_HIST_SLOTS + slot] = p;
    }
    unsigned long long *o = out + (long long)lo * YOLO2_HIST_WORDS;
    for (int b = tid; b < YOLO2_HIST_BUCKETS; b += Y2_HIST_THREADS) {
        const unsigned long long n = (unsigned long long)cnt[0][b] + cnt[1][b] + cnt[2][b] + cnt[3][b];
        if (n) atomicAdd(o + b, n);
    }
}

// one workgroup per job: its partials in slot order (thread t takes slots t, t + 256; butterfly; waves in order)
__global__ __launch_bounds__(Y2_HIST_THREADS) void hist_finalize_kernel(const yolo2_hist_job *__restrict__ jobs, unsigned long long *__restrict__ out,
                                                                         const Y2HistPartial *__restrict__ ws) {
    __shared__ double red[4][4];
    __shared__ unsigned long long nred[2];
    const int tid = threadIdx.x, wave = tid >> 6, j = blockIdx.x;
    const yolo2_hist_job job = jobs[j];
    const int nslots = y2_hist_slots(y2_hist_extent(job.rows, job.c, job.ld, job.dtype));
    if (tid < 2) nred[tid] = 0ull;
    __syncthreads();
    double mn = DBL_MAX, mx = -DBL_MAX, sum = 0.0, sq = 0.0;
    unsigned long long num = 0ull, nonfinite = 0ull;
    for (int s = tid; s < nslots; s += Y2_HIST_THREADS) {
        const Y2HistPartial p = ws[(long long)j * Y2_HIST_SLOTS + s];
        mn = p.mn < mn ? p.mn : mn;
        mx = p.mx > mx ? p.mx : mx;
        sum += p.sum;
        sq += p.sq;
        num += p.num;
        nonfinite += p.nonfinite;
    }
    sum = wave_sum_d(sum);
    sq = wave_sum_d(sq);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double m2 = __shfl_xor(mn, o, 64), x2 = __shfl_xor(mx, o, 64);
        mn = m2 < mn ? m2 : mn;
        mx = x2 > mx ? x2 : mx;
    }
    if ((tid & 63) == 0) { red[wave][0] = mn; red[wave][1] = mx; red[wave][2] = sum; red[wave][3] = sq; }
    if (num) atomicAdd(&nred[0], num);
    if (nonfinite) atomicAdd(&nred[1], nonfinite);
    __syncthreads();
    if (tid == 0) {
        double m = red[0][0], x = red[0][1];
        for (int w = 1; w < 4; ++w) { m = red[w][0] < m ? red[w][0] : m; x = red[w][1] > x ? red[w][1] : x; }
        double *stats = (double *)(out + (long long)j * YOLO2_HIST_WORDS + YOLO2_HIST_BUCKETS);
        stats[0] = m;
        stats[1] = x;
        stats[2] = ((red[0][2] + red[1][2]) + red[2][2]) + red[3][2];
        stats[3] = ((red[0][3] + red[1][3]) + red[2][3]) + red[3][3];
        unsigned long long *n = out + (long long)j * YOLO2_HIST_WORDS + YOLO2_HIST_BUCKETS + 4;
        n[0] = nred[0];
        n[1] = nred[1];
    }
}

extern "C" size_t yolo2_histogram_workspace_bytes(int njobs) { return (size_t)(njobs > 0 ? njobs : 0) * Y2_HIST_SLOTS * sizeof(Y2HistPartial); }
extern "C" size_t yolo2_histogram_result_bytes(int njobs) { return (size_t)(njobs > 0 ? njobs : 0) * YOLO2_HIST_WORDS * 8; }
extern "C" int yolo2_histogram_items(long long rows, int c, int ld, int dtype) { return y2_hist_slots(y2_hist_extent(rows, c, ld, dtype)); }

extern "C" int yolo2_histogram(const yolo2_hist_job *jobs, int njobs, int items, void *out, size_t out_bytes, void *ws, size_t ws_bytes, void *stream) {
    static_assert(sizeof(yolo2_hist_job) == 32 && sizeof(Y2HistPartial) == 48, "descriptor / partial layout");
    Y2_CHECK_ARG(jobs && out && ws && njobs > 0 && items >= 0 && (long long)items <= (long long)njobs * Y2_HIST_SLOTS);
    Y2_CHECK_ARG(out_bytes >= yolo2_histogram_result_bytes(njobs) && ws_bytes >= yolo2_histogram_workspace_bytes(njobs));
    Y2_CHECK_ARG(((uintptr_t)out & 7) == 0 && ((uintptr_t)ws & 7) == 0 && ((uintptr_t)jobs & 7) == 0);
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(out, 0, yolo2_histogram_result_bytes(njobs), st) != hipSuccess) { yolo2_set_error("yolo2_histogram: memset failed"); return YOLO2_E_LAUNCH; }
    if (items > 0) hist_bin_kernel<<<items, Y2_HIST_THREADS, 0, st>>>(jobs, njobs, (unsigned long long *)out, (Y2HistPartial *)ws);
    hist_finalize_kernel<<<njobs, Y2_HIST_THREADS, 0, st>>>(jobs, (unsigned long long *)out, (const Y2HistPartial *)ws);
    Y2_CHECK_LAUNCH();
    return YOLO2_OK;
}
