// Dimension clusters on gfx950: k-means over the ground-truth boxes' (w, h) with distance 1 - IoU (YOLO9000, section 2 "Dimension
// Clusters"; the reference lists it as the unchecked roadmap item README.md:88 and only ever reads the result, model/yolo2/__init__.py:106).
// New work: the reference has no such code, the semantics are those of include/yolo2_hip.h, section "dimension clusters".
//
// Many jobs (k, centroids) run in one launch.  One Lloyd iteration is two launches and nothing else: the assign kernel adds every
// box's contribution to its best centroid into a 64-bit INTEGER workspace (fixed point: integer adds commute, so the sums do not depend
// on the order workgroups arrive in and a fit is bitwise reproducible), the update kernel turns the sums into centroids, detects the
// fixed point, and clears the workspace again.  Iteration boundaries are launch boundaries: no workgroup waits for another.
//
// Assign, grid (box chunks, jobs), 256 lanes x 16 boxes: the boxes arrive as eight 16-byte loads per lane (two boxes each), all issued
// before the first use; the job's centroids are read through a pointer formed from blockIdx alone, so they are scalar loads and feed the
// VALU as scalar operands; the lane keeps best IoU and index of its 16 boxes in registers while it walks the k centroids.  IoU is f32 in the
// documented operation order with a correctly rounded division, FP contraction off; ties keep the lowest index (strict >).  Contributions
// meet in an LDS table of [kmax][3] + 1 64-bit words (LDS integer atomics), and the workgroup then issues one global 64-bit atomic add per
// non-zero word.  A 2^20-box job has 256 workgroups: at most 97 x 8 bytes of atomics each.
#include "common.h"
#pragma clang fp contract(off)

#define Y2_ANCHOR_THREADS 256
#define Y2_ANCHOR_LOADS 8                                              // 16-byte loads per lane
#define Y2_ANCHOR_BOXES (2 * Y2_ANCHOR_LOADS)                          // boxes per lane
#define Y2_ANCHOR_CHUNK (Y2_ANCHOR_THREADS * Y2_ANCHOR_BOXES)          // boxes per workgroup: 4096
#define Y2_ANCHOR_WORDS(kmax) (3 * (kmax) + 1)                         // per job: (count, sum w, sum h) per cluster, then the IoU sum

typedef unsigned long long u64;

__device__ __forceinline__ u64 anchor_fixed(float v, double scale) { return (u64)(long long)__builtin_rint((double)v * scale); }

// min of a lane's value and a wave-uniform one, neither NaN.  fminf() costs two instructions here: under IEEE mode the compiler quiets the
// vector operand with a v_max first, every time, because it cannot know that a loaded value is no signalling NaN.
__device__ __forceinline__ float anchor_min(float lane, float uniform) {
#if defined(__HIP_DEVICE_COMPILE__)
    float r;
    asm("v_min_f32 %0, %1, %2" : "=v"(r) : "s"(uniform), "v"(lane));
    return r;
#else
    return lane < uniform ? lane : uniform;
#endif
}

__global__ __launch_bounds__(Y2_ANCHOR_THREADS) void anchor_assign_kernel(const float *__restrict__ boxes, int n, const float *__restrict__ centroids,
                                                                           const int *__restrict__ job_k, int kmax, u64 *__restrict__ ws,
                                                                           const int *__restrict__ done, unsigned char *__restrict__ assignment) {
    __shared__ u64 table[Y2_ANCHOR_WORDS(YOLO2_ANCHOR_MAX_K)];
    const int job = blockIdx.y, tid = threadIdx.x;
    if (done && done[job]) return;                                     // a frozen job: nothing is added, so its workspace stays zero
    const int k = min(max(job_k[job], 1), kmax);
    const float *__restrict__ cen = centroids + (size_t)job * kmax * 2;         // wave-uniform: scalar loads
    const int words = Y2_ANCHOR_WORDS(kmax);
    for (int t = tid; t < words; t += Y2_ANCHOR_THREADS) table[t] = 0ull;

    // pair p = boxes 2p, 2p + 1; load i of this lane is pair first + i * 256 (consecutive lanes, consecutive 16 bytes)
    const long first = (long)blockIdx.x * (Y2_ANCHOR_CHUNK / 2) + tid;
    const long full = n >> 1;                                          // pairs that are wholly inside the array
    float w[Y2_ANCHOR_BOXES], h[Y2_ANCHOR_BOXES], area[Y2_ANCHOR_BOXES], best[Y2_ANCHOR_BOXES];
    int arg[Y2_ANCHOR_BOXES];
    f32x4 v[Y2_ANCHOR_LOADS];
    if ((long)(blockIdx.x + 1) * (Y2_ANCHOR_CHUNK / 2) <= full) {       // the whole chunk is inside (wave-uniform): eight loads in flight, no tests
#pragma unroll
        for (int i = 0; i < Y2_ANCHOR_LOADS; ++i) v[i] = *reinterpret_cast<const f32x4 *>(boxes + 4 * (first + (long)i * Y2_ANCHOR_THREADS));
    } else {
#pragma unroll
        for (int i = 0; i < Y2_ANCHOR_LOADS; ++i) {
            const long p = first + (long)i * Y2_ANCHOR_THREADS;
            v[i] = f32x4{1.f, 1.f, 1.f, 1.f};                          // past the end: a harmless box that is never accumulated
            if (p < full) v[i] = *reinterpret_cast<const f32x4 *>(boxes + 4 * p);
            else if (2 * p < n) { v[i][0] = boxes[4 * p]; v[i][1] = boxes[4 * p + 1]; }      // the last box of an odd n
        }
    }
#pragma unroll
    for (int i = 0; i < Y2_ANCHOR_LOADS; ++i) { w[2 * i] = v[i][0]; h[2 * i] = v[i][1]; w[2 * i + 1] = v[i][2]; h[2 * i + 1] = v[i][3]; }
#pragma unroll
    for (int i = 0; i < Y2_ANCHOR_BOXES; ++i) {
        area[i] = w[i] * h[i];
        best[i] = -1.f;
        arg[i] = 0;
    }
    for (int c = 0; c < k; ++c) {
        const float cw = cen[2 * c], ch = cen[2 * c + 1];                 // one s_load_dwordx2; the other waves of the SIMD cover its latency
        const float carea = cw * ch;
#pragma unroll
        for (int i = 0; i < Y2_ANCHOR_BOXES; ++i) {
            const float inter = anchor_min(w[i], cw) * anchor_min(h[i], ch);
            const float uni = (area[i] + carea) - inter;
            const float iou = inter / uni;
            if (iou > best[i]) { best[i] = iou; arg[i] = c; }          // strict: of equal overlaps the lowest index stays
        }
    }
    __syncthreads();                                                   // the table is zero
    u64 iou_sum = 0ull;
#pragma unroll
    for (int i = 0; i < Y2_ANCHOR_BOXES; ++i) {
        const long b = 2 * (first + (long)(i >> 1) * Y2_ANCHOR_THREADS) + (i & 1);
        if (b < n) {
            u64 *row = table + 3 * arg[i];
            atomicAdd(row, 1ull);
            atomicAdd(row + 1, anchor_fixed(w[i], 16777216.0));
            atomicAdd(row + 2, anchor_fixed(h[i], 16777216.0));
            iou_sum += anchor_fixed(best[i], 1073741824.0);
            if (assignment) assignment[(size_t)job * n + b] = (unsigned char)arg[i];
        }
    }
    if (iou_sum) atomicAdd(table + 3 * kmax, iou_sum);
    __syncthreads();
    u64 *slot = ws + (size_t)job * words;
    for (int t = tid; t < words; t += Y2_ANCHOR_THREADS) {
        const u64 add = table[t];
        if (add) __hip_atomic_fetch_add(slot + t, add, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// One wave per job.  Update pass (done given): new centroids from the sums, bitwise comparison, done / iterations; a frozen job returns
// at once.  Score pass (done NULL): centroids stay.  Either pass reports counts / avg_iou of the assignment it consumed when asked, and
// clears the job's workspace slots with plain stores.
__global__ __launch_bounds__(64) void anchor_update_kernel(float *__restrict__ centroids, const int *__restrict__ job_k, int kmax, u64 *__restrict__ ws,
                                                            int n, int *__restrict__ done, int *__restrict__ iterations,
                                                            long long *__restrict__ counts, double *__restrict__ avg_iou) {
    const int job = blockIdx.x, t = threadIdx.x;
    if (done && done[job]) return;
    const int k = min(max(job_k[job], 1), kmax);
    const int words = Y2_ANCHOR_WORDS(kmax);
    u64 *slot = ws + (size_t)job * words;
    long long cnt = 0, sw = 0, sh = 0;
    if (t < k) { cnt = (long long)slot[3 * t]; sw = (long long)slot[3 * t + 1]; sh = (long long)slot[3 * t + 2]; }
    const long long siou = (long long)slot[3 * kmax];
    __syncthreads();                                                   // every sum is in registers before a slot is cleared
    for (int i = t; i < words; i += 64) slot[i] = 0ull;
    if (done) {
        bool changed = false;
        if (t < k && cnt > 0) {                                        // an empty cluster keeps its centroid
            float *c = centroids + ((size_t)job * kmax + t) * 2;
            const float nw = (float)((double)sw / (double)cnt * 0x1p-24), nh = (float)((double)sh / (double)cnt * 0x1p-24);
            changed = __float_as_uint(nw) != __float_as_uint(c[0]) || __float_as_uint(nh) != __float_as_uint(c[1]);
            c[0] = nw; c[1] = nh;
        }
        const bool any = __ballot(changed) != 0ull;
        if (t == 0) {
            iterations[job] += 1;
            if (!any) done[job] = 1;
        }
    }
    if (counts && t < k) counts[(size_t)job * kmax + t] = cnt;
    if (avg_iou && t == 0) avg_iou[job] = (double)siou * 0x1p-30 / (double)n;
}

extern "C" size_t yolo2_anchor_workspace_bytes(int jobs, int kmax) {
    if (jobs < 1 || kmax < 1 || kmax > YOLO2_ANCHOR_MAX_K) return 0;
    return sizeof(u64) * (size_t)jobs * Y2_ANCHOR_WORDS(kmax);
}

static int anchor_check(const char *func, int n, int jobs, int kmax, const void *ws, size_t ws_bytes) {
    if (!(kmax >= 1 && kmax <= YOLO2_ANCHOR_MAX_K && jobs >= 1 && jobs <= YOLO2_ANCHOR_MAX_JOBS && n >= 1 && n <= YOLO2_ANCHOR_MAX_BOXES && ws &&
          ((uintptr_t)ws & 7) == 0 && ws_bytes >= yolo2_anchor_workspace_bytes(jobs, kmax))) {
        yolo2_set_error("%s: argument check failed: kmax %d (1..%d), jobs %d (1..%d), n %d (1..%d), ws %p of %zu bytes (needs %zu)", func, kmax,
                        YOLO2_ANCHOR_MAX_K, jobs, YOLO2_ANCHOR_MAX_JOBS, n, YOLO2_ANCHOR_MAX_BOXES, ws, ws_bytes,
                        yolo2_anchor_workspace_bytes(jobs, kmax));
        return YOLO2_E_ARG;
    }
    return YOLO2_OK;
}

extern "C" int yolo2_anchor_assign(const float *boxes, int n, const float *centroids, const int *job_k, int jobs, int kmax,
                                   unsigned long long *ws, size_t ws_bytes, const int *done, unsigned char *assignment, void *stream) {
    Y2_CHECK_ARG(boxes && centroids && job_k);
    Y2_CHECK_ARG(((uintptr_t)boxes & 15) == 0);
    if (int rc = anchor_check(__func__, n, jobs, kmax, ws, ws_bytes)) return rc;
    const dim3 grid(cdiv(n, Y2_ANCHOR_CHUNK), jobs);
    anchor_assign_kernel<<<grid, Y2_ANCHOR_THREADS, 0, (hipStream_t)stream>>>(boxes, n, centroids, job_k, kmax, ws, done, assignment);
    Y2_CHECK_LAUNCH();
    return YOLO2_OK;
}

extern "C" int yolo2_anchor_update(float *centroids, const int *job_k, int jobs, int kmax, unsigned long long *ws, size_t ws_bytes, int n,
                                   int *done, int *iterations, long long *counts, double *avg_iou, void *stream) {
    Y2_CHECK_ARG(job_k);
    Y2_CHECK_ARG((done != nullptr) == (iterations != nullptr));        // both: update pass; neither: score pass
    Y2_CHECK_ARG(done ? centroids != nullptr : (counts || avg_iou));
    if (int rc = anchor_check(__func__, n, jobs, kmax, ws, ws_bytes)) return rc;
    anchor_update_kernel<<<jobs, 64, 0, (hipStream_t)stream>>>(centroids, job_k, kmax, ws, n, done, iterations, counts, avg_iou);
    Y2_CHECK_LAUNCH();
    return YOLO2_OK;
}
