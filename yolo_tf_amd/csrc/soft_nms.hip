// Soft-NMS (Bodla et al., ICCV 2017) on gfx950: per class, the best remaining box is picked and the scores of the others decay by a function
// of their overlap with it -- hard (x 0 at IoU >= threshold_iou), linear (x (1 - IoU) there) or Gaussian (x soft_exp(-IoU^2 / sigma)) -- and
// the best is selected AGAIN after every decay.  The specification is tests/soft_nms_ref.py (NumPy float32), equal to this kernel bit for bit.
//
// One workgroup of 256 threads per (image, class); the classes are independent (a class reads and writes its own column only), so there
// is no snapshot and no workspace.  nms.hip's one sort + overlap bitmask does not carry over: the order changes with every pick.
//   1. compaction: the K candidates (score > threshold; NaN is none) go to LDS in box order -- score, box index, box: 24 bytes each.  The
//      waves take contiguous runs of 64-box chunks; a __ballot per chunk gives the counts (first pass) and the positions (second pass).
//      Box order is kept, so the compact position breaks score ties exactly as the box index does.  K = 0 ends the workgroup here.
//   2. the pick loop, one __syncthreads per pick: every thread owns the positions p = tid, tid + 256, ...; its key for the next pick is the
//      maximum over its live positions of (score bits << 32 | ~p) -- scores are >= +0, so their bit patterns order as unsigned integers,
//      and ~p prefers the lower position among equals.  A wave maximum (row rotations + permlane swaps, all VALU), one 8-byte LDS word per wave
//      (double-buffered by the pick's parity), and every thread knows the winner m.  If its score is not above the threshold the loop
//      ends; otherwise the owner of m negates its score (= picked; the value is final) and every thread decays its own live positions
//      against box m, taking its maximum for the NEXT pick in the same pass.  The key is a strict total order: the shape of the reduction
//      cannot matter.
//   3. write-back: picked -> the score, every other candidate -> +0.0f.  Non-candidates are never touched.
// A second launch (one workgroup per image, only with order_out) sorts the box indices by (max over classes of the final scores descending,
// index ascending) with nms.hip's bitonic network.
// IoU in nms.hip's operation order, f32, contraction off, subnormals kept (hipcc's default).  Boxes are finite with xy_min <= xy_max and areas
// that do not overflow: then 0 <= IoU <= 1 and every weight is in [0, 1], which the sign encoding of "picked" relies on.
#include "common.h"
#include "soft_exp.h"
#include "wave_max.h"
#include <atomic>
#include <math.h>
#pragma clang fp contract(off)

__device__ __forceinline__ u64 snms_key(float s, int p) { return ((u64)__builtin_bit_cast(unsigned, s) << 32) | (unsigned)~p; }

template <int METHOD>
__global__ __launch_bounds__(256) void soft_nms_kernel(float *__restrict__ conf, const float *__restrict__ xy_min, const float *__restrict__ xy_max,
                                                       int N, int C, float thr, float thr_iou, float sigma) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    f32x4 *sbox = reinterpret_cast<f32x4 *>(smem_raw);      // [N] (minx, miny, maxx, maxy) of compact position p; read-only after the compaction
    float *sc = reinterpret_cast<float *>(sbox + N);         // [N] current score; negated once picked.  Position p is touched by thread p % 256 only
    int *sidx = reinterpret_cast<int *>(sc + N);             // [N] compact position -> box index
    u64 *red = reinterpret_cast<u64 *>(sidx + N);            // [2][4] the waves' maxima, by the pick's parity (24 N is a multiple of 8)
    int *wcnt = reinterpret_cast<int *>(red + 8);            // [4] candidates per wave

    const int b = blockIdx.x / C, c = blockIdx.x % C;
    const long base = (long)b * N;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    // ---- 1. compaction, box order kept
    const int chunks = (N + 63) >> 6;
    const int cpw = (chunks + 3) >> 2;                       // 64-box chunks per wave
    const int ch0 = min(wave * cpw, chunks), ch1 = min(ch0 + cpw, chunks);
    int cnt = 0;
    for (int ch = ch0; ch < ch1; ++ch) {
        const int i = (ch << 6) + lane;
        const bool is = i < N && conf[(base + i) * C + c] > thr;
        cnt += __popcll(__ballot(is));
    }
    if (lane == 0) wcnt[wave] = cnt;
    __syncthreads();
    int pos = 0, K = 0;
    for (int w = 0; w < 4; ++w) {
        const int v = wcnt[w];
        pos += w < wave ? v : 0;
        K += v;
    }
    if (K == 0) return;
    for (int ch = ch0; ch < ch1; ++ch) {
        const int i = (ch << 6) + lane;
        const float s = i < N ? conf[(base + i) * C + c] : 0.0f;
        const bool is = i < N && s > thr;
        const u64 mask = __ballot(is);
        if (is) {
            const int p = pos + __popcll(mask & ((1ull << lane) - 1ull));
            f32x4 bx;
            bx[0] = xy_min[(base + i) * 2]; bx[1] = xy_min[(base + i) * 2 + 1];
            bx[2] = xy_max[(base + i) * 2]; bx[3] = xy_max[(base + i) * 2 + 1];
            sbox[p] = bx;
            sc[p] = s;
            sidx[p] = i;
        }
        pos += __popcll(mask);
    }
    __syncthreads();

    // ---- 2. the pick loop
    u64 best = 0ull;                                         // 0 = nothing live here (a key's low word ~p is never 0)
    for (int p = tid; p < K; p += 256) best = snms_max(best, snms_key(sc[p], p));
    for (int t = 0;; ++t) {
        best = snms_wave_max(best);
        u64 *slot = red + ((t & 1) << 2);
        if (lane == 0) slot[wave] = best;
        __syncthreads();
        const u64 k = snms_max(snms_max(slot[0], slot[1]), snms_max(slot[2], slot[3]));
        const float sm = __builtin_bit_cast(float, (unsigned)(k >> 32));
        if (!(sm > thr)) break;                              // (also: nothing live, k = 0)
        const int m = (int)~(unsigned)k;
        const f32x4 bm = sbox[m];
        const float a1 = (bm[2] - bm[0]) * (bm[3] - bm[1]);
        best = 0ull;
        for (int p = tid; p < K; p += 256) {
            float s = sc[p];
            if (p == m) { sc[p] = -s; continue; }            // picked: s > thr >= 0, so -s < 0
            if (s < 0.0f) continue;                          // picked earlier
            const f32x4 bq = sbox[p];
            const float a2 = (bq[2] - bq[0]) * (bq[3] - bq[1]);
            const float w = fmaxf(fminf(bm[2], bq[2]) - fmaxf(bm[0], bq[0]), 0.0f);
            const float h = fmaxf(fminf(bm[3], bq[3]) - fmaxf(bm[1], bq[1]), 0.0f);
            const float inter = w * h;
            const float iou = inter / fmaxf((a1 + a2) - inter, 1e-10f);
            float wt;
            if (METHOD == YOLO2_NMS_HARD) wt = iou >= thr_iou ? 0.0f : 1.0f;
            else if (METHOD == YOLO2_NMS_LINEAR) wt = iou >= thr_iou ? 1.0f - iou : 1.0f;
            else wt = soft_exp(-((iou * iou) / sigma));
            s = s * wt;
            sc[p] = s;
            best = snms_max(best, snms_key(s, p));
        }
    }

    // ---- 3. write-back (every thread its own positions)
    for (int p = tid; p < K; p += 256) {
        const float s = sc[p];
        conf[(base + sidx[p]) * C + c] = s < 0.0f ? -s : 0.0f;
    }
}

// order_out[b] = the box indices of image b by (max over classes of the final scores descending, box index ascending): nms.hip's bitonic network
// over perm[0..NP), padding (-1) last.  The comparator is a strict total order, so the result does not depend on the exchange order.
__global__ __launch_bounds__(256) void soft_nms_order_kernel(const float *__restrict__ conf, int *__restrict__ order_out, int N, int C, int NP) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    float *key = reinterpret_cast<float *>(smem_raw);        // [N]
    int *perm = reinterpret_cast<int *>(key + N);             // [NP]
    const long base = (long)blockIdx.x * N;
    const int tid = threadIdx.x;
    for (int i = tid; i < NP; i += 256) {
        perm[i] = i < N ? i : -1;
        if (i < N) {
            const float *row = conf + (base + i) * C;
            float m = row[0];
            for (int cc = 1; cc < C; ++cc) {
                const float v = row[cc];
                m = v > m ? v : m;
            }
            key[i] = m;
        }
    }
    for (int k = 2; k <= NP; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            __syncthreads();
            for (int t = tid; t < (NP >> 1); t += 256) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
                const int a = perm[i], bb = perm[l];
                bool b_first = false;
                if (bb >= 0) {
                    if (a < 0) b_first = true;
                    else {
                        const float ka = key[a], kb = key[bb];
                        b_first = kb != ka ? kb > ka : bb < a;
                    }
                }
                const bool up = (i & k) == 0;
                if (up == b_first && (a >= 0 || bb >= 0)) { perm[i] = bb; perm[l] = a; }
            }
        }
    __syncthreads();
    for (int p = tid; p < N; p += 256) order_out[base + p] = perm[p];
}

extern "C" int yolo2_soft_nms(float *conf, const float *xy_min, const float *xy_max, int *order_out, int B, int N, int C, int method,
                              float threshold, float threshold_iou, float sigma, void *stream) {
    Y2_CHECK_ARG(conf && xy_min && xy_max);
    Y2_CHECK_ARG(B > 0 && N > 0 && N <= 4096 && C > 0);
    Y2_CHECK_ARG(method == YOLO2_NMS_HARD || method == YOLO2_NMS_LINEAR || method == YOLO2_NMS_GAUSSIAN);
    Y2_CHECK_ARG(threshold >= 0.0f);                         // (false for NaN)
    Y2_CHECK_ARG(isfinite(threshold_iou));
    // sigma >= 1/64 keeps soft_exp's argument -IoU^2 / sigma above -65 (soft_exp.h)
    Y2_CHECK_ARG(method != YOLO2_NMS_GAUSSIAN || (isfinite(sigma) && sigma >= 0.015625f));
    hipStream_t st = (hipStream_t)stream;
    const void *kernel = method == YOLO2_NMS_HARD ? (const void *)soft_nms_kernel<YOLO2_NMS_HARD>
                       : method == YOLO2_NMS_LINEAR ? (const void *)soft_nms_kernel<YOLO2_NMS_LINEAR> : (const void *)soft_nms_kernel<YOLO2_NMS_GAUSSIAN>;
    const size_t lds = 24 * (size_t)N + 8 * 8 + 4 * 4;       // <= 98384 bytes at N = 4096
    if (lds > 64 * 1024) {
        // the attribute is per device and per kernel: remember what each has been raised to, as yolo2_nms does
        static std::atomic<size_t> lds_set[3][64];
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = -1;
        if (dev < 0 || lds > lds_set[method][dev].load(std::memory_order_relaxed)) {
            if (hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
                yolo2_set_error("soft_nms: cannot reserve %zu bytes of LDS", lds);
                return YOLO2_E_LAUNCH;
            }
            if (dev >= 0) lds_set[method][dev].store(lds, std::memory_order_relaxed);
        }
    }
    if (method == YOLO2_NMS_HARD) soft_nms_kernel<YOLO2_NMS_HARD><<<B * C, 256, lds, st>>>(conf, xy_min, xy_max, N, C, threshold, threshold_iou, sigma);
    else if (method == YOLO2_NMS_LINEAR) soft_nms_kernel<YOLO2_NMS_LINEAR><<<B * C, 256, lds, st>>>(conf, xy_min, xy_max, N, C, threshold, threshold_iou, sigma);
    else soft_nms_kernel<YOLO2_NMS_GAUSSIAN><<<B * C, 256, lds, st>>>(conf, xy_min, xy_max, N, C, threshold, threshold_iou, sigma);
    Y2_CHECK_LAUNCH();
    if (order_out) {
        int NP = 2;
        while (NP < N) NP <<= 1;
        soft_nms_order_kernel<<<B, 256, sizeof(float) * (size_t)N + sizeof(int) * (size_t)NP, st>>>(conf, order_out, N, C, NP);      // <= 32 KB
        Y2_CHECK_LAUNCH();
    }
    return YOLO2_OK;
}
