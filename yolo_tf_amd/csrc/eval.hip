// Detection scoring on gfx950: PASCAL VOC average precision of the boxes a DetectSession leaves on the device
// (include/yolo2_hip.h, section "evaluation").  Integer / LDS / bandwidth work, no MFMA; wave64 throughout.
//
// Stage A (yolo2_eval_collect, once per detect batch, three launches, no host synchronisation):
//   eval_count_kernel  one workgroup per image: the number of detections of the image (mode `detect`: one per box whose first arg-max
//                      score exceeds the threshold; mode `all`: one per (box, class) score above it).
//   eval_emit_kernel   one workgroup per image.  The image's ground truth sits in LDS.  Append position = records wanted so far
//                      (device word) + the counts of the earlier images of the batch + the rank inside the image, which comes from
//                      __ballot / popcount prefixes in (box, class) order: no position depends on the arrival order of an atomic.
//                      VOC matching needs the detections of an (image, class) in (score desc, box asc) order only to decide which of the
//                      detections that claim one ground truth box is the first: the candidate of a detection (highest IoU, lowest index
//                      on ties, matched or not) does not depend on the others.  So pass 1 takes, per ground truth box, the MINIMUM of the
//                      order keys of the detections that claim it (64-bit LDS atomicMin: a minimum is the same in any arrival order),
//                      and pass 2 recomputes each candidate with the same instructions and flags the detection TP when its key is that
//                      minimum, FP (duplicate) when it is not, ignored when the candidate is difficult, FP when nothing overlaps enough.
//   eval_bump_kernel   adds the batch's count to the device word.
// Stage B (yolo2_eval_finalize, once per evaluation):
//   LSD radix sort of the 16-byte records (eval_sort.h, shared with eval_coco.hip), 8 bits per pass (histogram per 16384-record tile, one-workgroup scan of the digit x tile
//   table, stable scatter), over box index, image index, inverted score bits and class key: the result is ordered by (class, score
//   desc, image asc, box asc) whatever the order of the collect calls.  Ignored records carry class key C + class and sort behind.
//   eval_ap_kernel, one workgroup per class: binary search of the class segment, integer scans of TP / FP over per-thread contiguous
//   ranges, precision / recall in f64, the 11 VOC2007 maxima, and the VOC2012 area from a backward walk that carries the running
//   maximum of the precision.  Every f64 sum has a fixed association, so two runs give the same bits.
// IoU is f32 in the reference's operation order ((a1+a2)-inter, floor 1e-10; utils/postprocess.py:21-36) with FP contraction off, as
// in nms.hip.
#include "eval_sort.h"
#pragma clang fp contract(off)

#define EV_AP_THREADS 1024

__global__ __launch_bounds__(256) void eval_count_kernel(const float *__restrict__ conf, int *__restrict__ counts, int N, int C, float thr, int mode) {
    __shared__ int sred[4];
    const int b = blockIdx.x;
    const float *cb = conf + (long)b * N * C;
    const int items = mode == YOLO2_EVAL_MODE_ALL ? N * C : N;
    int n = 0, box, cls;
    float score;
    for (int it = threadIdx.x; it < items; it += 256) n += ev_item(cb, it, items, C, thr, mode, box, cls, score) ? 1 : 0;
    n = ev_block_sum(n, sred);
    if (threadIdx.x == 0) counts[b] = n;
}

__global__ __launch_bounds__(256) void eval_emit_kernel(const float *__restrict__ conf, const float *__restrict__ xy_min, const float *__restrict__ xy_max,
                                                        const int *__restrict__ gt_class, const float *__restrict__ gt_box,
                                                        const unsigned char *__restrict__ gt_difficult, const int *__restrict__ gt_first, int G,
                                                        const int *__restrict__ counts, unsigned long long *__restrict__ state, int *__restrict__ npos,
                                                        u32x4 *__restrict__ records, long capacity, int N, int C, float thr, float thr_iou,
                                                        int mode, int image_base) {
    __shared__ f32x4 sbox[YOLO2_EVAL_MAX_GT_PER_IMAGE];
    __shared__ unsigned long long skey[YOLO2_EVAL_MAX_GT_PER_IMAGE];
    __shared__ int scls[YOLO2_EVAL_MAX_GT_PER_IMAGE];
    __shared__ unsigned char sdiff[YOLO2_EVAL_MAX_GT_PER_IMAGE];
    __shared__ int sred[4];
    __shared__ int swave[4];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g0 = gt_first[b], g1 = gt_first[b + 1];
    int ng = g1 - g0;
    if (g0 < 0 || g1 < g0 || g1 > G || ng > YOLO2_EVAL_MAX_GT_PER_IMAGE) {
        if (tid == 0) atomicOr(&state[1], EV_ERR_GT_FIRST);
        ng = 0;
    }
    for (int g = tid; g < ng; g += 256) {
        const float *p = gt_box + (long)(g0 + g) * 4;
        f32x4 bx;
        bx[0] = p[0]; bx[1] = p[1]; bx[2] = p[2]; bx[3] = p[3];
        sbox[g] = bx;
        int c = gt_class[g0 + g];
        const unsigned char d = gt_difficult[g0 + g];
        if (c < 0 || c >= C) {
            atomicOr(&state[1], EV_ERR_GT_CLASS);
            c = -1;                                        // matches no detection
        } else if (!d) {
            atomicAdd(&npos[c], 1);                        // integer: the sum does not depend on the order
        }
        scls[g] = c;
        sdiff[g] = d;
        skey[g] = ~0ull;
    }
    int before = 0;
    for (int i = tid; i < b; i += 256) before += counts[i];
    before = ev_block_sum(before, sred);                   // (also the barrier behind the LDS fill)
    const long base = (long)state[0] + before;

    const float *cb = conf + (long)b * N * C;
    const int items = mode == YOLO2_EVAL_MODE_ALL ? N * C : N;
    // the candidate of a detection: highest IoU among the image's ground truth of its class, lowest index on ties
    auto candidate = [&](int box, int cls, float &best) {
        f32x4 d;
        d[0] = xy_min[((long)b * N + box) * 2]; d[1] = xy_min[((long)b * N + box) * 2 + 1];
        d[2] = xy_max[((long)b * N + box) * 2]; d[3] = xy_max[((long)b * N + box) * 2 + 1];
        int arg = -1;
        best = 0.0f;
        for (int g = 0; g < ng; ++g) {
            if (scls[g] != cls) continue;
            const float iou = ev_iou(d, sbox[g]);
            if (arg < 0 || iou > best) { best = iou; arg = g; }
        }
        return arg;
    };
    auto order_key = [](float score, int box) { return ((unsigned long long)(~ev_ord(score)) << 32) | (unsigned)box; };
    // pass 1: per ground truth box, the first (score desc, box asc) of the detections that claim it
    for (int it = tid; it < items; it += 256) {
        int box, cls;
        float score, iou;
        if (!ev_item(cb, it, items, C, thr, mode, box, cls, score)) continue;
        const int g = candidate(box, cls, iou);
        if (g >= 0 && iou > thr_iou && !sdiff[g]) atomicMin(&skey[g], order_key(score, box));
    }
    __syncthreads();
    // pass 2: flag and append in (box, class) order
    int run = 0;
    for (int it0 = 0; it0 < items; it0 += 256) {
        int box = 0, cls = 0;
        float score = 0.0f;
        const bool keep = ev_item(cb, it0 + tid, items, C, thr, mode, box, cls, score);
        const unsigned long long mask = __ballot(keep);
        if (lane == 0) swave[wave] = __popcll(mask);
        __syncthreads();
        int off = 0, total = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const int v = swave[w];
            off += w < wave ? v : 0;
            total += v;
        }
        if (keep) {
            const long pos = base + run + off + __popcll(mask & ((1ull << lane) - 1ull));
            float iou;
            const int g = candidate(box, cls, iou);
            unsigned flag = YOLO2_EVAL_FP;
            if (g >= 0 && iou > thr_iou) {
                if (sdiff[g]) flag = YOLO2_EVAL_IGNORED;
                else if (skey[g] == order_key(score, box)) flag = YOLO2_EVAL_TP;
            }
            if (pos < capacity) {                           // never past the end: the needed count is kept, yolo2_eval_finalize reports it
                u32x4 r;
                r[0] = __builtin_bit_cast(unsigned, score);
                r[1] = (unsigned)(image_base + b);
                r[2] = (unsigned)box;
                r[3] = ((unsigned)cls << 2) | flag;
                records[pos] = r;
            }
        }
        run += total;
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void eval_bump_kernel(const int *__restrict__ counts, int n, unsigned long long *__restrict__ state) {
    __shared__ int sred[4];
    int t = 0;
    for (int i = threadIdx.x; i < n; i += 256) t += counts[i];
    t = ev_block_sum(t, sred);
    if (threadIdx.x == 0) state[0] = state[0] + (unsigned long long)t;
}

// ---- stage B ----------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned ev_class_key(unsigned cf, int C) {
    const unsigned cls = cf >> 2;
    return (cf & 3u) == YOLO2_EVAL_IGNORED ? (unsigned)C + cls : cls;
}
struct ev_voc_field {                    // the sort fields of a yolo2_eval_record (eval_sort.h)
    static __device__ __forceinline__ unsigned get(const u32x4 r, int field, int C) {
        switch (field) {
        case 0: return r[2];
        case 1: return r[1];
        case 2: return ~ev_ord(__builtin_bit_cast(float, r[0]));      // descending score
        default: return ev_class_key(r[3], C);
        }
    }
    static __device__ __forceinline__ bool bad(const u32x4 r, int n_images, int N, int C) {
        return r[1] >= (unsigned)n_images || r[2] >= (unsigned)N || (r[3] >> 2) >= (unsigned)C;
    }
};

__device__ __forceinline__ long ev_lower_bound(const u32x4 *__restrict__ recs, long M, unsigned key, int C) {
    long a = 0, b = M;
    while (a < b) {
        const long m = (a + b) >> 1;
        if (ev_class_key(recs[m][3], C) < key) a = m + 1;
        else b = m;
    }
    return a;
}
__device__ __forceinline__ double ev_wave_max(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}

// results (8-byte words): ap07 [C] f64, ap12 [C] f64, npos [C], tp [C], fp [C], ignored [C] i64, records held, records needed, error bits
__global__ __launch_bounds__(EV_AP_THREADS) void eval_ap_kernel(const u32x4 *__restrict__ recs, const unsigned long long *__restrict__ state, long capacity,
                                                                const int *__restrict__ npos_in, int C, unsigned long long *__restrict__ results,
                                                                int *__restrict__ cum_tp, int *__restrict__ cum_fp) {
    __shared__ int stp[EV_AP_THREADS], sfp[EV_AP_THREADS];
    __shared__ double smax[EV_AP_THREADS];
    __shared__ double swm[11][EV_AP_THREADS / 64];
    const int c = blockIdx.x, tid = threadIdx.x;
    const long M = ev_count(state, capacity);
    const long s = ev_lower_bound(recs, M, (unsigned)c, C), e = ev_lower_bound(recs, M, (unsigned)c + 1u, C);
    const long is = ev_lower_bound(recs, M, (unsigned)(C + c), C), ie = ev_lower_bound(recs, M, (unsigned)(C + c) + 1u, C);
    const long L = e - s, per = (L + EV_AP_THREADS - 1) / EV_AP_THREADS;
    const long lo = s + min((long)tid * per, L), hi = s + min((long)(tid + 1) * per, L);
    const int npos = npos_in[c];
    int tpc = 0, fpc = 0;
    for (long i = lo; i < hi; ++i) {
        const bool tp = (recs[i][3] & 3u) == YOLO2_EVAL_TP;
        tpc += tp ? 1 : 0;
        fpc += tp ? 0 : 1;
    }
    stp[tid] = tpc;
    sfp[tid] = fpc;
    __syncthreads();
    int tp0 = 0, fp0 = 0, tp_all = 0, fp_all = 0;
    for (int t = 0; t < EV_AP_THREADS; ++t) {
        const int a = stp[t], b = sfp[t];
        tp0 += t < tid ? a : 0;
        fp0 += t < tid ? b : 0;
        tp_all += a;
        fp_all += b;
    }
    // forward walk: cumulative counts, precision / recall, the 11 maxima, this range's highest precision
    double m[11], pmax = 0.0;
#pragma unroll
    for (int k = 0; k < 11; ++k) m[k] = 0.0;
    {
        int tp = tp0, fp = fp0;
        for (long i = lo; i < hi; ++i) {
            const bool t = (recs[i][3] & 3u) == YOLO2_EVAL_TP;
            tp += t ? 1 : 0;
            fp += t ? 0 : 1;
            if (cum_tp) cum_tp[i] = tp;
            if (cum_fp) cum_fp[i] = fp;
            if (npos > 0) {
                const double prec = (double)tp / (double)(tp + fp), rec = (double)tp / (double)npos;
                pmax = fmax(pmax, prec);
#pragma unroll
                for (int k = 0; k < 11; ++k)
                    if (rec >= (double)k / 10.0) m[k] = fmax(m[k], prec);
            }
        }
    }
    smax[tid] = pmax;
#pragma unroll
    for (int k = 0; k < 11; ++k) {
        const double v = ev_wave_max(m[k]);
        if ((tid & 63) == 0) swm[k][tid >> 6] = v;
    }
    __syncthreads();
    // backward walk: the precision envelope (running maximum from the end) times the recall step of every TP
    double carry = 0.0, part = 0.0;
    for (int t = tid + 1; t < EV_AP_THREADS; ++t) carry = fmax(carry, smax[t]);
    if (npos > 0) {
        int tp = tp0 + tpc, fp = fp0 + fpc;
        for (long i = hi - 1; i >= lo; --i) {
            const bool t = (recs[i][3] & 3u) == YOLO2_EVAL_TP;
            carry = fmax(carry, (double)tp / (double)(tp + fp));
            if (t) part += ((double)tp / (double)npos - (double)(tp - 1) / (double)npos) * carry;
            tp -= t ? 1 : 0;
            fp -= t ? 0 : 1;
        }
    }
    __syncthreads();                     // (smax is read above, rewritten below)
    smax[tid] = part;
    __syncthreads();
    if (tid == 0) {
        double ap12 = 0.0, ap07 = 0.0;
        for (int t = 0; t < EV_AP_THREADS; ++t) ap12 += smax[t];           // fixed order
        for (int k = 0; k < 11; ++k) {
            double v = 0.0;
            for (int w = 0; w < EV_AP_THREADS / 64; ++w) v = fmax(v, swm[k][w]);
            ap07 += v;
        }
        ap07 = ap07 / 11.0;
        if (npos <= 0) ap07 = ap12 = __builtin_nan("");
        results[c] = __builtin_bit_cast(unsigned long long, ap07);
        results[C + c] = __builtin_bit_cast(unsigned long long, ap12);
        results[2 * C + c] = (unsigned long long)(long long)npos;
        results[3 * C + c] = (unsigned long long)tp_all;
        results[4 * C + c] = (unsigned long long)fp_all;
        results[5 * C + c] = (unsigned long long)(ie - is);
        if (c == 0) {
            results[6 * C] = (unsigned long long)M;
            results[6 * C + 1] = state[0];
            results[6 * C + 2] = state[1];
        }
    }
}


extern "C" size_t yolo2_eval_record_bytes(long max_records) { return max_records > 0 ? (size_t)max_records * sizeof(yolo2_eval_record) : 0; }
extern "C" size_t yolo2_eval_collect_workspace_bytes(int B) { return B > 0 ? (size_t)B * sizeof(int) : 0; }
extern "C" size_t yolo2_eval_workspace_bytes(long max_records, int C) {
    if (max_records <= 0 || C <= 0) return 0;
    return 2 * ev_align((size_t)max_records * sizeof(yolo2_eval_record)) + ev_align((size_t)ev_tiles(max_records) * 256 * sizeof(int));
}
extern "C" size_t yolo2_eval_result_bytes(int C) { return C > 0 ? (size_t)(6 * (size_t)C + 3) * 8 : 0; }

extern "C" int yolo2_eval_collect(const float *conf, const float *xy_min, const float *xy_max, const int *gt_class, const float *gt_box,
                                  const unsigned char *gt_difficult, const int *gt_first, int G, int B, int N, int C, int n_valid, int image_base,
                                  int mode, float threshold, float iou_threshold, void *records, long max_records, unsigned long long *state,
                                  int *npos, int *ws, void *stream) {
    Y2_CHECK_ARG(conf && xy_min && xy_max && gt_class && gt_box && gt_difficult && gt_first && records && state && npos && ws);
    Y2_CHECK_ARG(B > 0 && N > 0 && C > 0 && C <= YOLO2_EVAL_MAX_CLASSES && (long)N * C <= 0x7FFFFFFFL);
    Y2_CHECK_ARG(G >= 0 && n_valid >= 0 && n_valid <= B && image_base >= 0 && (long)image_base + B <= 0x7FFFFFFFL);
    Y2_CHECK_ARG(mode == YOLO2_EVAL_MODE_DETECT || mode == YOLO2_EVAL_MODE_ALL);
    Y2_CHECK_ARG(max_records > 0 && max_records <= 0x7FFFFFFFL);
    Y2_CHECK_ARG(threshold == threshold && iou_threshold == iou_threshold);
    if (n_valid == 0) return YOLO2_OK;
    hipStream_t st = (hipStream_t)stream;
    eval_count_kernel<<<n_valid, 256, 0, st>>>(conf, ws, N, C, threshold, mode);
    Y2_CHECK_LAUNCH();
    eval_emit_kernel<<<n_valid, 256, 0, st>>>(conf, xy_min, xy_max, gt_class, gt_box, gt_difficult, gt_first, G, ws, state, npos, (u32x4 *)records,
                                              max_records, N, C, threshold, iou_threshold, mode, image_base);
    Y2_CHECK_LAUNCH();
    eval_bump_kernel<<<1, 256, 0, st>>>(ws, n_valid, state);
    Y2_CHECK_LAUNCH();
    return YOLO2_OK;
}

extern "C" int yolo2_eval_finalize(const void *records, long max_records, unsigned long long *state, const int *npos, int C, int n_images, int N,
                                   void *ws, size_t ws_bytes, void *results, void *sorted_records, int *cum_tp, int *cum_fp, void *stream) {
    Y2_CHECK_ARG(records && state && npos && ws && results);
    Y2_CHECK_ARG(C > 0 && C <= YOLO2_EVAL_MAX_CLASSES && n_images > 0 && N > 0);
    Y2_CHECK_ARG(max_records > 0 && max_records <= 0x7FFFFFFFL);
    Y2_CHECK_ARG(ws_bytes >= yolo2_eval_workspace_bytes(max_records, C));
    hipStream_t st = (hipStream_t)stream;
    const size_t rec_bytes = ev_align((size_t)max_records * sizeof(yolo2_eval_record));
    u32x4 *buf[2] = {(u32x4 *)ws, (u32x4 *)((char *)ws + rec_bytes)};
    int *table = (int *)((char *)ws + 2 * rec_bytes);
    const int tiles = (int)ev_tiles(max_records);
    // least significant digit first: box, image, inverted score, class key (0 .. 2C-1: ignored records sort behind as C + class)
    struct { int field, bytes; } keys[4] = {{0, ev_bytes_for((unsigned long long)N - 1)}, {1, ev_bytes_for((unsigned long long)n_images - 1)}, {2, 4},
                                            {3, ev_bytes_for(2ull * C - 1)}};
    const u32x4 *src = (const u32x4 *)records;
    int which = 0, first = 1;
    for (int k = 0; k < 4; ++k)
        for (int byte = 0; byte < keys[k].bytes; ++byte) {
            eval_hist_kernel<ev_voc_field><<<tiles, 256, 0, st>>>(src, state, max_records, table, keys[k].field, 8 * byte, C, first, n_images, N);
            Y2_CHECK_LAUNCH();
            eval_scan_kernel<<<1, 256, 0, st>>>(table, tiles);
            Y2_CHECK_LAUNCH();
            eval_scatter_kernel<ev_voc_field><<<tiles, 256, 0, st>>>(src, buf[which], state, max_records, table, keys[k].field, 8 * byte, C);
            Y2_CHECK_LAUNCH();
            src = buf[which];
            which ^= 1;
            first = 0;
        }
    eval_ap_kernel<<<C, EV_AP_THREADS, 0, st>>>(src, state, max_records, npos, C, (unsigned long long *)results, cum_tp, cum_fp);
    Y2_CHECK_LAUNCH();
    if (sorted_records && hipMemcpyAsync(sorted_records, src, (size_t)max_records * sizeof(yolo2_eval_record), hipMemcpyDeviceToDevice, st) != hipSuccess) {
        yolo2_set_error("eval_finalize: copy of the sorted records failed");
        return YOLO2_E_LAUNCH;
    }
    return YOLO2_OK;
}
