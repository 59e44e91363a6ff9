// Detection scoring on gfx950, COCO protocol (include/yolo2_hip.h, section "evaluation, COCO protocol"): AP / AR over IoU thresholds,
// area ranges and detection limits of the boxes a DetectSession leaves on the device.  Integer / LDS work, no MFMA; wave64 throughout.
//
// Stage A (yolo2_eval_coco_collect, once per detect batch, three launches, no host synchronisation):
//   coco_count_kernel  one workgroup per image: detections per class (integer LDS atomics: a count does not depend on the arrival
//                      order), the kept count min(n, max_dets) per class, its exclusive prefix over the classes and the image's total.
//                      Mode `detect` also leaves (class, score) of every box in the workspace, so the arg-max runs once.
//   coco_match_kernel  one workgroup per image, its ground truth in LDS, one wave per class in turn; a class without a detection in
//                      the image is skipped after reading its count.  The wave compacts the class's detections in box order (ballot /
//                      popcount) into 64-bit order keys (inverted score bits << 32 | box: smaller = earlier), finds each key's rank by
//                      counting the keys below it (64 keys per load, broadcast lane by lane: deterministic, no sort) and drops the keys
//                      of rank < max_dets into an LDS slot array.  COCO's matching is greedy and sequential in rank order, but the
//                      A * T <= 40 (area range, IoU threshold) walks are independent: lane a * T + t runs one.  Per detection the wave
//                      first writes the IoU row against the class's boxes into LDS (lane k computes box k), then every lane scans that
//                      row -- non-ignored boxes of ITS area range, then the ignored ones -- against its own matched bits
//                      (smatch[word][lane]: the lanes of a wave touch 64 consecutive words, no bank conflict).  Two ballots turn the
//                      lanes' outcomes into the record's `matched` and `ignored` bit sets.  Append position = records wanted so far
//                      + kept counts of the earlier images + kept prefix of the earlier classes + rank: counts and prefixes only.
//   coco_bump_kernel   adds the batch's kept count to the device word.
// Stage B (yolo2_eval_coco_finalize, once per evaluation):
//   coco_key_kernel builds a 16-byte sort key per record (score bits, image, record index, class << 8 | rank); the radix passes of
//   eval_sort.h order the keys by (class, score desc, image asc, rank asc); coco_ap_kernel, one workgroup per (class, slice, IoU
//   threshold), walks the class segment in per-thread contiguous ranges: integer scans of TP / FP among the records that are below the
//   slice's detection limit and not ignored, precision in f64, a backward walk that carries the running maximum of the precision and
//   drops it into q[r] for the recall thresholds r each true positive is the first to reach; thread 0 adds q[0..R) in index order.
#include "eval_sort.h"
#pragma clang fp contract(off)

#define CO_THREADS 256
#define CO_WAVES 4
#define CO_GT YOLO2_EVAL_MAX_GT_PER_IMAGE

struct co_tables {                               // by value in the kernel arguments: nothing is copied or synchronised
    float lo[YOLO2_EVAL_COCO_MAX_AREAS], hi[YOLO2_EVAL_COCO_MAX_AREAS], thr[YOLO2_EVAL_COCO_MAX_IOUS];
    int A, T;
};
struct co_final {
    double rec[YOLO2_EVAL_COCO_MAX_RECALLS];
    int slice_area[YOLO2_EVAL_COCO_MAX_SLICES], slice_limit[YOLO2_EVAL_COCO_MAX_SLICES];
    int R, S;
};
struct co_ws {                                   // the collect workspace
    int *counts, *cls_cnt, *cls_off, *det_cls;
    float *det_score;
    unsigned long long *scratch;
    size_t bytes;
};
static co_ws co_layout(void *ws, int B, int N, int C) {
    char *p = (char *)ws;
    size_t o = 0;
    co_ws w;
    auto take = [&](size_t n) { char *q = p + o; o += ev_align(n); return q; };
    w.counts = (int *)take((size_t)B * 4);
    w.cls_cnt = (int *)take((size_t)B * C * 4);
    w.cls_off = (int *)take((size_t)B * C * 4);
    w.det_cls = (int *)take((size_t)B * N * 4);
    w.det_score = (float *)take((size_t)B * N * 4);
    w.scratch = (unsigned long long *)take((size_t)B * CO_WAVES * N * 8);
    w.bytes = o;
    return w;
}

__global__ __launch_bounds__(CO_THREADS) void coco_count_kernel(const float *__restrict__ conf, co_ws ws, int N, int C, float thr, int mode, int max_dets) {
    __shared__ int scnt[YOLO2_EVAL_COCO_MAX_CLASSES];
    __shared__ int spart[CO_THREADS];
    const int b = blockIdx.x, tid = threadIdx.x;
    for (int c = tid; c < C; c += CO_THREADS) scnt[c] = 0;
    __syncthreads();
    const float *cb = conf + (long)b * N * C;
    const int items = mode == YOLO2_EVAL_MODE_ALL ? N * C : N;
    for (int it = tid; it < items; it += CO_THREADS) {
        int box, cls;
        float score;
        const bool keep = ev_item(cb, it, items, C, thr, mode, box, cls, score);
        if (keep) atomicAdd(&scnt[cls], 1);
        if (mode == YOLO2_EVAL_MODE_DETECT) {
            ws.det_cls[(long)b * N + it] = keep ? cls : -1;
            ws.det_score[(long)b * N + it] = score;
        }
    }
    __syncthreads();
    const int per = (C + CO_THREADS - 1) / CO_THREADS;
    const int c0 = min(tid * per, C), c1 = min(c0 + per, C);
    int sum = 0;
    for (int c = c0; c < c1; ++c) sum += min(scnt[c], max_dets);
    spart[tid] = sum;
    __syncthreads();
    int off = 0, total = 0;
    for (int t = 0; t < CO_THREADS; ++t) {
        const int v = spart[t];
        off += t < tid ? v : 0;
        total += v;
    }
    for (int c = c0; c < c1; ++c) {
        ws.cls_cnt[(long)b * C + c] = scnt[c];
        ws.cls_off[(long)b * C + c] = off;
        off += min(scnt[c], max_dets);
    }
    if (tid == 0) ws.counts[b] = total;
}

// the wave's LDS writes become visible to its other lanes (the compiler keeps the order, the LDS queue is in order)
__device__ __forceinline__ void co_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__global__ __launch_bounds__(CO_THREADS) void coco_match_kernel(const float *__restrict__ conf, const float *__restrict__ xy_min, const float *__restrict__ xy_max,
                                                                const int *__restrict__ gt_class, const float *__restrict__ gt_box,
                                                                const float *__restrict__ gt_area, const unsigned char *__restrict__ gt_flags,
                                                                const int *__restrict__ gt_first, const float *__restrict__ scale, int G, co_ws ws,
                                                                unsigned long long *__restrict__ state, int *__restrict__ npig,
                                                                yolo2_eval_coco_record *__restrict__ records, long capacity, int N, int C, float thr,
                                                                int mode, int image_base, int max_dets, co_tables tab) {
    __shared__ f32x4 sbox[CO_GT];
    __shared__ float sarea[CO_GT];
    __shared__ int scls[CO_GT];
    __shared__ unsigned char sflag[CO_GT];
    __shared__ unsigned short sgl[CO_WAVES][CO_GT];                  // the class's boxes, index order
    __shared__ unsigned char sign[CO_WAVES][CO_GT];                  // bit a: ignored under area range a; bit 7: crowd
    __shared__ unsigned smatch[CO_WAVES][CO_GT / 32][64];            // [word][lane]: bit k of lane (a, t) = box k is taken at (a, t)
    __shared__ float siou[CO_WAVES][CO_GT];
    __shared__ unsigned long long sslot[CO_WAVES][YOLO2_EVAL_COCO_MAX_DETS];
    __shared__ unsigned long long sres[CO_WAVES][YOLO2_EVAL_COCO_MAX_DETS][2];
    __shared__ float slo[YOLO2_EVAL_COCO_MAX_AREAS], shi[YOLO2_EVAL_COCO_MAX_AREAS], sthr[YOLO2_EVAL_COCO_MAX_IOUS];
    __shared__ int sred[4];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int A = tab.A, T = tab.T;
    if (tid < YOLO2_EVAL_COCO_MAX_AREAS) {
        slo[tid] = tab.lo[tid];
        shi[tid] = tab.hi[tid];
    }
    if (tid < YOLO2_EVAL_COCO_MAX_IOUS) sthr[tid] = tab.thr[tid];
    const int g0 = gt_first[b], g1 = gt_first[b + 1];
    int ng = g1 - g0;
    if (g0 < 0 || g1 < g0 || g1 > G || ng > CO_GT) {
        if (tid == 0) atomicOr(&state[1], EV_ERR_GT_FIRST);
        ng = 0;
    }
    __syncthreads();
    for (int g = tid; g < ng; g += CO_THREADS) {
        const float *p = gt_box + (long)(g0 + g) * 4;
        f32x4 bx;
        bx[0] = p[0]; bx[1] = p[1]; bx[2] = p[2]; bx[3] = p[3];
        sbox[g] = bx;
        int c = gt_class[g0 + g];
        const float area = gt_area[g0 + g];
        const unsigned char fl = gt_flags[g0 + g];
        if (c < 0 || c >= C) {
            atomicOr(&state[1], EV_ERR_GT_CLASS);
            c = -1;                                        // matches no detection
        } else {
            for (int a = 0; a < A; ++a)
                if (!((fl & 3) || area < slo[a] || area > shi[a])) atomicAdd(&npig[a * C + c], 1);      // integer: any order, one sum
        }
        scls[g] = c;
        sarea[g] = area;
        sflag[g] = fl;
    }
    int before = 0;
    for (int i = tid; i < b; i += CO_THREADS) before += ws.counts[i];
    before = ev_block_sum(before, sred);                   // (also the barrier behind the LDS fill)
    const long base = (long)state[0] + before;
    const float sx = scale[b * 2], sy = scale[b * 2 + 1];
    unsigned long long *list = ws.scratch + ((long)b * CO_WAVES + wave) * N;
    const unsigned long long below = (1ull << lane) - 1ull;
    const bool active = lane < A * T;
    const int la = active ? lane / T : 0, lt = active ? lane - la * T : 0;

    for (int c = wave; c < C; c += CO_WAVES) {
        const int n_c = ws.cls_cnt[(long)b * C + c];
        if (n_c == 0) continue;                             // (uniform for the wave)
        const int n_keep = min(n_c, max_dets), off = ws.cls_off[(long)b * C + c];
        // the class's detections as order keys, box order
        int run = 0;
        for (int i0 = 0; i0 < N; i0 += 64) {
            const int i = i0 + lane;
            bool is = false;
            float sc = 0.0f;
            if (i < N) {
                if (mode == YOLO2_EVAL_MODE_ALL) {
                    sc = conf[((long)b * N + i) * C + c] + 0.0f;
                    is = sc > thr;
                } else {
                    is = ws.det_cls[(long)b * N + i] == c;
                    sc = ws.det_score[(long)b * N + i];
                }
            }
            const unsigned long long mask = __ballot(is);
            if (is) list[run + __popcll(mask & below)] = ((unsigned long long)(~ev_ord(sc)) << 32) | (unsigned)i;
            run += __popcll(mask);
        }
        __threadfence_block();                              // the list is read back by other lanes of this wave
        // rank = the number of keys below mine; the first max_dets land in rank order
        for (int m0 = 0; m0 < n_c; m0 += 64) {
            const bool valid = m0 + lane < n_c;
            const unsigned long long my = valid ? list[m0 + lane] : ~0ull;
            int rank = 0;
            for (int t0 = 0; t0 < n_c; t0 += 64) {
                const unsigned long long tk = t0 + lane < n_c ? list[t0 + lane] : ~0ull;
                const int kmax = min(64, n_c - t0);
                for (int k = 0; k < kmax; ++k) rank += __shfl(tk, k, 64) < my ? 1 : 0;
            }
            if (valid && rank < n_keep) sslot[wave][rank] = my;
        }
        // the class's ground truth, index order, and its ignore bits per area range
        int ngc = 0;
        for (int q0 = 0; q0 < ng; q0 += 64) {
            const int g = q0 + lane;
            const bool is = g < ng && scls[g] == c;
            const unsigned long long mask = __ballot(is);
            if (is) {
                const int k = ngc + __popcll(mask & below);
                const float area = sarea[g];
                const unsigned fl = sflag[g];
                unsigned bits = (fl & 2) ? 0x80u : 0u;
                for (int a = 0; a < A; ++a) bits |= ((fl & 3) || area < slo[a] || area > shi[a]) ? 1u << a : 0u;
                sgl[wave][k] = (unsigned short)g;
                sign[wave][k] = (unsigned char)bits;
            }
            ngc += __popcll(mask);
        }
        for (int w = 0; w < (ngc + 31) / 32; ++w) smatch[wave][w][lane] = 0u;
        co_wave_sync();
        for (int r = 0; r < n_keep; ++r) {
            const unsigned long long key = sslot[wave][r];
            const long at = ((long)b * N + (unsigned)key) * 2;
            f32x4 d;
            d[0] = xy_min[at]; d[1] = xy_min[at + 1];
            d[2] = xy_max[at]; d[3] = xy_max[at + 1];
            const float dw = d[2] - d[0], dh = d[3] - d[1];
            const float dcell = dw * dh, dpx = (dw * sx) * (dh * sy);
            for (int k = lane; k < ngc; k += 64) {         // the IoU row, once for all (a, t)
                const f32x4 q = sbox[sgl[wave][k]];
                float v;
                if (sign[wave][k] & 0x80u) {
                    const float w = fmaxf(fminf(d[2], q[2]) - fmaxf(d[0], q[0]), 0.0f);
                    const float h = fmaxf(fminf(d[3], q[3]) - fmaxf(d[1], q[1]), 0.0f);
                    v = (w * h) / fmaxf(dcell, 1e-10f);
                } else {
                    v = ev_iou(d, q);
                }
                siou[wave][k] = v;
            }
            co_wave_sync();
            int m = -1;
            if (active) {
                double best = fmin((double)sthr[lt], 1.0 - 1e-10);
                for (int pass = 0; pass < 2 && m < 0; ++pass)      // an ignored box is looked at only when no other one matched
                    for (int k = 0; k < ngc; ++k) {
                        const unsigned bits = sign[wave][k];
                        if ((int)((bits >> la) & 1u) != pass) continue;
                        if (((smatch[wave][k >> 5][lane] >> (k & 31)) & 1u) && !(bits & 0x80u)) continue;
                        const double v = (double)siou[wave][k];
                        if (v < best) continue;
                        best = v;                               // >=: of equal overlaps the last one in scan order wins
                        m = k;
                    }
            }
            bool ign;
            if (m >= 0) {
                ign = (sign[wave][m] >> la) & 1u;
                smatch[wave][m >> 5][lane] |= 1u << (m & 31);
            } else {
                ign = dpx < slo[la] || dpx > shi[la];
            }
            const unsigned long long mb = __ballot(active && m >= 0), ib = __ballot(active && ign);
            if (lane == 0) {
                sres[wave][r][0] = mb;
                sres[wave][r][1] = ib;
            }
            co_wave_sync();
        }
        for (int r = lane; r < n_keep; r += 64) {
            const long pos = base + off + r;
            if (pos < capacity) {                           // never past the end: the needed count is kept, finalize reports it
                const unsigned long long key = sslot[wave][r];
                yolo2_eval_coco_record rec;
                rec.score = ev_unord(~(unsigned)(key >> 32));
                rec.image = image_base + b;
                rec.box = (int)(unsigned)key;
                rec.cls = c;
                rec.rank = r;
                rec.reserved = 0u;
                rec.matched = sres[wave][r][0];
                rec.ignored = sres[wave][r][1];
                records[pos] = rec;
            }
        }
        co_wave_sync();                                     // (the slots and results are rewritten by the next class)
    }
}

__global__ __launch_bounds__(CO_THREADS) void coco_bump_kernel(const int *__restrict__ counts, int n, unsigned long long *__restrict__ state) {
    __shared__ int sred[4];
    int t = 0;
    for (int i = threadIdx.x; i < n; i += CO_THREADS) t += counts[i];
    t = ev_block_sum(t, sred);
    if (threadIdx.x == 0) state[0] = state[0] + (unsigned long long)t;
}

// ---- stage B ----------------------------------------------------------------------------------------------------------------------
struct co_key_field {                    // sort key: [0] score bits, [1] image, [2] record index, [3] class << 8 | rank
    static __device__ __forceinline__ unsigned get(const u32x4 r, int field, int) {
        switch (field) {
        case 0: return r[3] & 255u;
        case 1: return r[1];
        case 2: return ~ev_ord(__builtin_bit_cast(float, r[0]));      // descending score
        default: return r[3] >> 8;
        }
    }
    static __device__ __forceinline__ bool bad(const u32x4 r, int n_images, int max_dets, int C) {
        return r[1] >= (unsigned)n_images || (r[3] & 255u) >= (unsigned)max_dets || (r[3] >> 8) >= (unsigned)C;
    }
};

__global__ __launch_bounds__(256) void coco_key_kernel(const yolo2_eval_coco_record *__restrict__ records, unsigned long long *__restrict__ state,
                                                       long capacity, u32x4 *__restrict__ keys, int C, int N, int max_dets) {
    const long M = ev_count(state, capacity);
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= M) return;
    const yolo2_eval_coco_record r = records[i];
    // (a class or rank outside its range would not fit its key field: it is flagged here and clamped, so the sort stays in bounds)
    const bool bad = (unsigned)r.cls >= (unsigned)C || (unsigned)r.rank >= (unsigned)max_dets || (unsigned)r.box >= (unsigned)N;
    if (bad) atomicOr(&state[1], EV_ERR_RECORD);
    u32x4 k;
    k[0] = __builtin_bit_cast(unsigned, r.score);
    k[1] = (unsigned)r.image;
    k[2] = (unsigned)i;
    k[3] = bad ? 0u : ((unsigned)r.cls << 8) | (unsigned)r.rank;
    keys[i] = k;
}

__device__ __forceinline__ long co_lower_bound(const u32x4 *__restrict__ keys, long M, unsigned cls) {
    long a = 0, b = M;
    while (a < b) {
        const long m = (a + b) >> 1;
        if ((keys[m][3] >> 8) < cls) a = m + 1;
        else b = m;
    }
    return a;
}
// the number of recall thresholds (ascending) that are <= v
__device__ __forceinline__ int co_upper(const double *rec, int R, double v) {
    int a = 0, b = R;
    while (a < b) {
        const int m = (a + b) >> 1;
        if (rec[m] <= v) a = m + 1;
        else b = m;
    }
    return a;
}

// results (8-byte words): ap [S][T][C] f64, recall [S][T][C] f64, npig [A][C] i64, records held, records needed, error bits
__global__ __launch_bounds__(CO_THREADS) void coco_ap_kernel(const u32x4 *__restrict__ keys, const yolo2_eval_coco_record *__restrict__ records,
                                                             const unsigned long long *__restrict__ state, long capacity, const int *__restrict__ npig,
                                                             int C, int A, int T, co_final fin, unsigned long long *__restrict__ results) {
    __shared__ int stp[CO_THREADS], sfp[CO_THREADS];
    __shared__ double smax[CO_THREADS];
    __shared__ double srec[YOLO2_EVAL_COCO_MAX_RECALLS], sq[YOLO2_EVAL_COCO_MAX_RECALLS];
    const int c = blockIdx.x, s = blockIdx.y, t = blockIdx.z, tid = threadIdx.x;
    const int R = fin.R, S = fin.S, a = fin.slice_area[s], limit = fin.slice_limit[s], bit = a * T + t;
    for (int r = tid; r < R; r += CO_THREADS) {
        srec[r] = fin.rec[r];
        sq[r] = 0.0;
    }
    const long M = ev_count(state, capacity);
    const long s0 = co_lower_bound(keys, M, (unsigned)c), e0 = co_lower_bound(keys, M, (unsigned)c + 1u);
    const long L = e0 - s0, per = (L + CO_THREADS - 1) / CO_THREADS;
    const long lo = s0 + min((long)tid * per, L), hi = s0 + min((long)(tid + 1) * per, L);
    const int np = npig[a * C + c];
    // 0: not counted (beyond the slice's detection limit, or ignored at (a, t)); 1: false positive; 2: true positive
    auto kind = [&](long i) {
        const u32x4 k = keys[i];
        if ((int)(k[3] & 255u) >= limit) return 0;
        const yolo2_eval_coco_record *r = records + k[2];
        if ((r->ignored >> bit) & 1ull) return 0;
        return (int)((r->matched >> bit) & 1ull) + 1;
    };
    int tpc = 0, fpc = 0;
    for (long i = lo; i < hi; ++i) {
        const int k = kind(i);
        tpc += k == 2 ? 1 : 0;
        fpc += k == 1 ? 1 : 0;
    }
    stp[tid] = tpc;
    sfp[tid] = fpc;
    __syncthreads();
    int tp0 = 0, fp0 = 0, tp_all = 0, fp_all = 0;
    for (int u = 0; u < CO_THREADS; ++u) {
        const int x = stp[u], y = sfp[u];
        tp0 += u < tid ? x : 0;
        fp0 += u < tid ? y : 0;
        tp_all += x;
        fp_all += y;
    }
    const double eps = 2.220446049250313e-16;
    double pmax = 0.0;
    if (np > 0) {
        int tp = tp0, fp = fp0;
        for (long i = lo; i < hi; ++i) {
            const int k = kind(i);
            if (k == 0) continue;
            tp += k == 2 ? 1 : 0;
            fp += k == 1 ? 1 : 0;
            pmax = fmax(pmax, (double)tp / (((double)fp + (double)tp) + eps));
        }
    }
    smax[tid] = pmax;
    __syncthreads();
    // backward walk: the precision envelope (running maximum from the end).  The first counted record whose inclusive TP count is n
    // is the first point with recall >= r for every threshold r in (recall(n - 1), recall(n)]; the very first counted record also
    // serves every r <= recall(0) = 0.
    if (np > 0) {
        double carry = 0.0;
        for (int u = tid + 1; u < CO_THREADS; ++u) carry = fmax(carry, smax[u]);
        int tp = tp0 + tpc, fp = fp0 + fpc;
        for (long i = hi - 1; i >= lo; --i) {
            const int k = kind(i);
            if (k == 0) continue;
            carry = fmax(carry, (double)tp / (((double)fp + (double)tp) + eps));
            const bool first = tp + fp == 1;
            if (k == 2 || first) {
                const int r1 = co_upper(srec, R, (double)tp / (double)np);
                const int r0 = first ? 0 : co_upper(srec, R, (double)(tp - 1) / (double)np);
                for (int r = r0; r < r1; ++r) sq[r] = carry;          // (each r is written by one thread only)
            }
            tp -= k == 2 ? 1 : 0;
            fp -= k == 1 ? 1 : 0;
        }
    }
    __syncthreads();
    if (tid == 0) {
        double ap = 0.0;
        for (int r = 0; r < R; ++r) ap += sq[r];                       // fixed order
        ap = ap / (double)R;
        double rc = tp_all + fp_all > 0 ? (double)tp_all / (double)np : 0.0;
        if (np <= 0) ap = rc = -1.0;
        const long STC = (long)S * T * C;
        results[((long)s * T + t) * C + c] = __builtin_bit_cast(unsigned long long, ap);
        results[STC + ((long)s * T + t) * C + c] = __builtin_bit_cast(unsigned long long, rc);
        if (s == 0 && t == 0) {
            for (int x = 0; x < A; ++x) results[2 * STC + (long)x * C + c] = (unsigned long long)(long long)npig[x * C + c];
            if (c == 0) {
                results[2 * STC + (long)A * C] = (unsigned long long)M;
                results[2 * STC + (long)A * C + 1] = state[0];
                results[2 * STC + (long)A * C + 2] = state[1];
            }
        }
    }
}

static bool co_dims_ok(int A, int T, int C, int max_dets) {
    return A > 0 && A <= YOLO2_EVAL_COCO_MAX_AREAS && T > 0 && T <= YOLO2_EVAL_COCO_MAX_IOUS && C > 0 && C <= YOLO2_EVAL_COCO_MAX_CLASSES &&
           max_dets > 0 && max_dets <= YOLO2_EVAL_COCO_MAX_DETS;
}

extern "C" size_t yolo2_eval_coco_record_bytes(long max_records) { return max_records > 0 ? (size_t)max_records * sizeof(yolo2_eval_coco_record) : 0; }
extern "C" size_t yolo2_eval_coco_collect_workspace_bytes(int B, int N, int C) {
    if (B <= 0 || N <= 0 || C <= 0) return 0;
    return co_layout(nullptr, B, N, C).bytes;
}
extern "C" size_t yolo2_eval_coco_workspace_bytes(long max_records, int C) {
    if (max_records <= 0 || C <= 0) return 0;
    return 2 * ev_align((size_t)max_records * sizeof(u32x4)) + ev_align((size_t)ev_tiles(max_records) * 256 * sizeof(int));
}
extern "C" size_t yolo2_eval_coco_result_bytes(int S, int T, int A, int C) {
    if (S <= 0 || T <= 0 || A <= 0 || C <= 0) return 0;
    return (2 * (size_t)S * T * C + (size_t)A * C + 3) * 8;
}

extern "C" int yolo2_eval_coco_collect(const float *conf, const float *xy_min, const float *xy_max, const int *gt_class, const float *gt_box,
                                       const float *gt_area, const unsigned char *gt_flags, const int *gt_first, const float *scale, int G, int B,
                                       int N, int C, int n_valid, int image_base, int mode, float threshold, const float *area_ranges, int A,
                                       const float *iou_thresholds, int T, int max_dets, void *records, long max_records,
                                       unsigned long long *state, int *npig, void *ws, size_t ws_bytes, void *stream) {
    Y2_CHECK_ARG(conf && xy_min && xy_max && gt_class && gt_box && gt_area && gt_flags && gt_first && scale && records && state && npig && ws);
    Y2_CHECK_ARG(area_ranges && iou_thresholds);
    Y2_CHECK_ARG(B > 0 && N > 0 && (long)N * C <= 0x7FFFFFFFL && (long)B * N <= 0x7FFFFFFFL);
    Y2_CHECK_ARG(co_dims_ok(A, T, C, max_dets));
    Y2_CHECK_ARG(G >= 0 && n_valid >= 0 && n_valid <= B && image_base >= 0 && (long)image_base + B <= 0x7FFFFFFFL);
    Y2_CHECK_ARG(mode == YOLO2_EVAL_MODE_DETECT || mode == YOLO2_EVAL_MODE_ALL);
    Y2_CHECK_ARG(max_records > 0 && max_records <= 0x7FFFFFFFL);
    Y2_CHECK_ARG(threshold == threshold);
    Y2_CHECK_ARG(ws_bytes >= yolo2_eval_coco_collect_workspace_bytes(B, N, C));
    co_tables tab = {};
    tab.A = A;
    tab.T = T;
    for (int a = 0; a < A; ++a) {
        tab.lo[a] = area_ranges[2 * a];
        tab.hi[a] = area_ranges[2 * a + 1];
        Y2_CHECK_ARG(tab.lo[a] == tab.lo[a] && tab.hi[a] == tab.hi[a]);
    }
    for (int t = 0; t < T; ++t) {
        tab.thr[t] = iou_thresholds[t];
        Y2_CHECK_ARG(tab.thr[t] == tab.thr[t]);
    }
    if (n_valid == 0) return YOLO2_OK;
    hipStream_t st = (hipStream_t)stream;
    const co_ws w = co_layout(ws, B, N, C);
    coco_count_kernel<<<n_valid, CO_THREADS, 0, st>>>(conf, w, N, C, threshold, mode, max_dets);
    Y2_CHECK_LAUNCH();
    coco_match_kernel<<<n_valid, CO_THREADS, 0, st>>>(conf, xy_min, xy_max, gt_class, gt_box, gt_area, gt_flags, gt_first, scale, G, w, state, npig,
                                                      (yolo2_eval_coco_record *)records, max_records, N, C, threshold, mode, image_base, max_dets, tab);
    Y2_CHECK_LAUNCH();
    coco_bump_kernel<<<1, CO_THREADS, 0, st>>>(w.counts, n_valid, state);
    Y2_CHECK_LAUNCH();
    return YOLO2_OK;
}

extern "C" int yolo2_eval_coco_finalize(const void *records, long max_records, unsigned long long *state, const int *npig, int C, int n_images, int N,
                                        int A, int T, int max_dets, const int *slices, int S, const double *recall_thresholds, int R, void *ws,
                                        size_t ws_bytes, void *results, void *stream) {
    Y2_CHECK_ARG(records && state && npig && ws && results && slices && recall_thresholds);
    Y2_CHECK_ARG(co_dims_ok(A, T, C, max_dets) && n_images > 0 && N > 0);
    Y2_CHECK_ARG(S > 0 && S <= YOLO2_EVAL_COCO_MAX_SLICES && R > 0 && R <= YOLO2_EVAL_COCO_MAX_RECALLS);
    Y2_CHECK_ARG(max_records > 0 && max_records <= 0x7FFFFFFFL);
    Y2_CHECK_ARG(ws_bytes >= yolo2_eval_coco_workspace_bytes(max_records, C));
    co_final fin = {};
    fin.R = R;
    fin.S = S;
    for (int s = 0; s < S; ++s) {
        fin.slice_area[s] = slices[2 * s];
        fin.slice_limit[s] = slices[2 * s + 1];
        Y2_CHECK_ARG(fin.slice_area[s] >= 0 && fin.slice_area[s] < A && fin.slice_limit[s] > 0 && fin.slice_limit[s] <= max_dets);
    }
    for (int r = 0; r < R; ++r) {
        fin.rec[r] = recall_thresholds[r];
        Y2_CHECK_ARG(fin.rec[r] == fin.rec[r] && (r == 0 || fin.rec[r] >= fin.rec[r - 1]));      // no NaN, ascending
    }
    hipStream_t st = (hipStream_t)stream;
    const size_t key_bytes = ev_align((size_t)max_records * sizeof(u32x4));
    u32x4 *buf[2] = {(u32x4 *)ws, (u32x4 *)((char *)ws + key_bytes)};
    int *table = (int *)((char *)ws + 2 * key_bytes);
    const int tiles = (int)ev_tiles(max_records);
    const yolo2_eval_coco_record *recs = (const yolo2_eval_coco_record *)records;
    coco_key_kernel<<<(unsigned)((max_records + 255) / 256), 256, 0, st>>>(recs, state, max_records, buf[0], C, N, max_dets);
    Y2_CHECK_LAUNCH();
    // least significant digit first: rank, image, inverted score, class
    struct { int field, bytes; } keys[4] = {{0, 1}, {1, ev_bytes_for((unsigned long long)n_images - 1)}, {2, 4}, {3, ev_bytes_for((unsigned long long)C - 1)}};
    int which = 0, first = 1;
    for (int k = 0; k < 4; ++k)
        for (int byte = 0; byte < keys[k].bytes; ++byte) {
            eval_hist_kernel<co_key_field><<<tiles, 256, 0, st>>>(buf[which], state, max_records, table, keys[k].field, 8 * byte, C, first, n_images, max_dets);
            Y2_CHECK_LAUNCH();
            eval_scan_kernel<<<1, 256, 0, st>>>(table, tiles);
            Y2_CHECK_LAUNCH();
            eval_scatter_kernel<co_key_field><<<tiles, 256, 0, st>>>(buf[which], buf[which ^ 1], state, max_records, table, keys[k].field, 8 * byte, C);
            Y2_CHECK_LAUNCH();
            which ^= 1;
            first = 0;
        }
    coco_ap_kernel<<<dim3(C, S, T), CO_THREADS, 0, st>>>(buf[which], recs, state, max_records, npig, C, A, T, fin, (unsigned long long *)results);
    Y2_CHECK_LAUNCH();
    return YOLO2_OK;
}
