// Test-time augmentation on gfx950: the boxes of several views of one image (sizes, mirror) are brought into the base view's grid
// (yolo2_tta_gather) and fused per class by Weighted Boxes Fusion (Solovyev, Wang, Gabruseva 2021; unit view weights, conf_type = avg)
// in yolo2_wbf.  The specification is tests/tta_ref.py (NumPy float32), equal to these kernels bit for bit.
//
// gather: one elementwise launch per view, one thread per (image, box, class); the thread of class 0 also moves the box.
//
// fuse: one workgroup of 256 threads per (image, class), as soft_nms.hip; the classes are independent.
//   1. compaction: the K candidates (score > threshold; NaN is none) are counted with one __ballot per 64-box chunk, and their keys
//      (score bits << 32 | ~pooled index) go to LDS at the positions the ballots give.  K = 0 ends the workgroup (count 0); K above
//      YOLO2_WBF_MAX_CANDIDATES sets flag bit 0 and ends it too.
//   2. sort: a bitonic network over the keys, padded with 0 to a power of two, descending.  Scores are > threshold >= +0, so their bit
//      patterns order as unsigned integers and ~index prefers the lower index among equals: a strict total order.  The boxes are then
//      fetched into LDS in sorted order.
//   3. the walk, one __syncthreads per candidate: thread t owns the clusters t, t + 256, ...; it computes the candidate's IoU with the
//      CURRENT FUSED box of each (nms.hip's operation order, the cluster in the place of the picked box) and keeps the maximum of
//      (IoU bits << 32 | ~cluster index).  IoU >= +0, so again a strict total order: a wave maximum (wave_max.h), one 8-byte LDS word per wave
//      (double-buffered by the candidate's parity), and every thread knows the best cluster.  Its owner adds the candidate (one multiply
//      and one add per coordinate, S += s, T += 1, four divisions) or the owner of the next free slot opens a cluster whose fused box is
//      the candidate's box itself.  A cluster is read and written by its owner only, so the reduction's barrier is the only one.  The
//      next candidate's key and box are loaded before the barrier.  More than max_per_class clusters: flag bit 1, count 0.
//   4. every owner writes its clusters' boxes and scores ((S / T) * min(T, V)) / V to the workspace; thread 0 writes the count.
// emit: one workgroup per image zeroes the image's R rows, takes the prefix sum of the C counts in class order (256 classes at a time, a
//   scan in LDS) and writes row r of class c: the score in column c, the box.  rows[b] = min(total, R); more than R sets flag bit 2.
// flags is OR-ed with atomicOr (a vector atomic); nothing waits on another workgroup.
//
// LDS of the fuse kernel (dynamic; Kcap = min(M, YOLO2_WBF_MAX_CANDIDATES), NP = the power of two >= Kcap, P = max_per_class):
//     keys      8 NP        sorted (score, ~index)
//     boxes    16 Kcap      (minx, miny, maxx, maxy) in sorted order
//     fused    16 P         the clusters' current boxes
//     sums     16 P         sum of score * coordinate
//     S, T      8 P         sum of scores, member count
//     red, cnt  64 + 16     the waves' maxima (two parities), the waves' candidate counts
// = 24 * 4096 + 40 * 1024 + 80 = 139,344 bytes at the caps, inside the 160 KiB (163,840 bytes) one workgroup may use on gfx950; a
// detector's usual M (a few thousand) and P = 256 take 24 M + 10 KB, so several workgroups share a CU.
#include "common.h"
#include "wave_max.h"
#include <atomic>
#include <math.h>
#pragma clang fp contract(off)

__global__ __launch_bounds__(256) void tta_gather_kernel(const float *__restrict__ conf, const float *__restrict__ xy_min, const float *__restrict__ xy_max,
                                                         float *__restrict__ out_conf, float *__restrict__ out_xy_min, float *__restrict__ out_xy_max,
                                                         long total, int N, int C, int M, int offset, float sx, float sy, float w0, int flip) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const int c = (int)(t % C);
    const long bi = t / C;                                   // b * N + i
    const long row = (bi / N) * M + offset + bi % N;         // b * M + offset + i
    out_conf[row * C + c] = conf[t];
    if (c == 0) {
        const float x0 = xy_min[bi * 2], y0 = xy_min[bi * 2 + 1], x1 = xy_max[bi * 2], y1 = xy_max[bi * 2 + 1];
        out_xy_min[row * 2] = flip ? w0 - x1 * sx : x0 * sx;
        out_xy_max[row * 2] = flip ? w0 - x0 * sx : x1 * sx;
        out_xy_min[row * 2 + 1] = y0 * sy;
        out_xy_max[row * 2 + 1] = y1 * sy;
    }
}

__global__ __launch_bounds__(256) void wbf_fuse_kernel(const float *__restrict__ conf, const float *__restrict__ xy_min, const float *__restrict__ xy_max,
                                                       int *__restrict__ counts, f32x4 *__restrict__ rec_box, float *__restrict__ rec_score, int *flags,
                                                       int M, int C, int V, int P, int Kcap, int NP, float thr, float fuse_iou) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    u64 *skey = reinterpret_cast<u64 *>(smem_raw);           // [NP] (8 NP is a multiple of 16: NP >= 2)
    f32x4 *sbox = reinterpret_cast<f32x4 *>(skey + NP);      // [Kcap]
    f32x4 *cbox = sbox + Kcap;                               // [P] fused boxes
    f32x4 *csum = cbox + P;                                  // [P] sums of score * coordinate
    float *cS = reinterpret_cast<float *>(csum + P);         // [P]
    int *cT = reinterpret_cast<int *>(cS + P);               // [P]
    u64 *red = reinterpret_cast<u64 *>(smem_raw + 8 * (size_t)NP + 16 * (size_t)Kcap + 40 * (size_t)P);      // [2][4]
    int *wcnt = reinterpret_cast<int *>(red + 8);            // [4]

    const int bc = blockIdx.x, b = bc / C, c = bc % C;
    const long base = (long)b * M;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    // ---- 1. compaction
    const int chunks = (M + 63) >> 6;
    const int cpw = (chunks + 3) >> 2;
    const int ch0 = min(wave * cpw, chunks), ch1 = min(ch0 + cpw, chunks);
    int cnt = 0;
    for (int ch = ch0; ch < ch1; ++ch) {
        const int i = (ch << 6) + lane;
        const bool is = i < M && conf[(base + i) * C + c] > thr;
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
    if (K == 0 || K > YOLO2_WBF_MAX_CANDIDATES) {            // (K <= M always, so K <= Kcap below)
        if (tid == 0) {
            counts[bc] = 0;
            if (K) atomicOr(flags, YOLO2_WBF_FLAG_CANDIDATES);
        }
        return;
    }
    int NK = 1;
    while (NK < K) NK <<= 1;
    for (int ch = ch0; ch < ch1; ++ch) {
        const int i = (ch << 6) + lane;
        const float s = i < M ? conf[(base + i) * C + c] : 0.0f;
        const bool is = i < M && s > thr;
        const u64 mask = __ballot(is);
        if (is) skey[pos + __popcll(mask & ((1ull << lane) - 1ull))] = ((u64)__builtin_bit_cast(unsigned, s) << 32) | (unsigned)~i;
        pos += __popcll(mask);
    }
    for (int p = K + tid; p < NK; p += 256) skey[p] = 0ull;  // padding sorts last (a key's low word ~i is never 0)

    // ---- 2. sort, descending
    for (int k = 2; k <= NK; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            __syncthreads();
            for (int t = tid; t < (NK >> 1); t += 256) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
                const u64 a = skey[i], bb = skey[l];
                if (((i & k) == 0) ? a < bb : a > bb) { skey[i] = bb; skey[l] = a; }
            }
        }
    __syncthreads();
    for (int p = tid; p < K; p += 256) {
        const long i = base + (int)~(unsigned)skey[p];
        f32x4 bx;
        bx[0] = xy_min[i * 2]; bx[1] = xy_min[i * 2 + 1];
        bx[2] = xy_max[i * 2]; bx[3] = xy_max[i * 2 + 1];
        sbox[p] = bx;
    }
    __syncthreads();

    // ---- 3. the walk
    int ncl = 0;
    u64 kq = skey[0];
    f32x4 q = sbox[0];
    for (int t = 0; t < K; ++t) {
        const float s = __builtin_bit_cast(float, (unsigned)(kq >> 32));
        const float a2 = (q[2] - q[0]) * (q[3] - q[1]);
        u64 best = 0ull;
        for (int j = tid; j < ncl; j += 256) {
            const f32x4 bm = cbox[j];
            const float a1 = (bm[2] - bm[0]) * (bm[3] - bm[1]);
            const float w = fmaxf(fminf(bm[2], q[2]) - fmaxf(bm[0], q[0]), 0.0f);
            const float h = fmaxf(fminf(bm[3], q[3]) - fmaxf(bm[1], q[1]), 0.0f);
            const float inter = w * h;
            const float iou = inter / fmaxf((a1 + a2) - inter, 1e-10f);
            best = snms_max(best, ((u64)__builtin_bit_cast(unsigned, iou) << 32) | (unsigned)~j);
        }
        const int tn = min(t + 1, K - 1);                    // the next candidate, ahead of the barrier
        const u64 kn = skey[tn];
        const f32x4 qn = sbox[tn];
        best = snms_wave_max(best);
        u64 *slot = red + ((t & 1) << 2);
        if (lane == 0) slot[wave] = best;
        __syncthreads();
        const u64 k = snms_max(snms_max(slot[0], slot[1]), snms_max(slot[2], slot[3]));
        const int m = (int)~(unsigned)k;
        const bool join = ncl > 0 && __builtin_bit_cast(float, (unsigned)(k >> 32)) >= fuse_iou;
        if (join) {
            if (tid == (m & 255)) {
                f32x4 sum = csum[m];
                sum[0] = sum[0] + s * q[0];
                sum[1] = sum[1] + s * q[1];
                sum[2] = sum[2] + s * q[2];
                sum[3] = sum[3] + s * q[3];
                const float S = cS[m] + s;
                csum[m] = sum;
                cS[m] = S;
                cT[m] = cT[m] + 1;
                f32x4 fb;
                fb[0] = sum[0] / S; fb[1] = sum[1] / S; fb[2] = sum[2] / S; fb[3] = sum[3] / S;
                cbox[m] = fb;
            }
        } else {
            if (ncl == P) {                                  // (uniform)
                if (tid == 0) {
                    counts[bc] = 0;
                    atomicOr(flags, YOLO2_WBF_FLAG_CLUSTERS);
                }
                return;
            }
            if (tid == (ncl & 255)) {
                f32x4 sum;
                sum[0] = s * q[0]; sum[1] = s * q[1]; sum[2] = s * q[2]; sum[3] = s * q[3];
                cbox[ncl] = q;
                csum[ncl] = sum;
                cS[ncl] = s;
                cT[ncl] = 1;
            }
            ++ncl;
        }
        kq = kn;
        q = qn;
    }

    // ---- 4. the records (every owner its own clusters)
    const float fv = (float)V;
    for (int j = tid; j < ncl; j += 256) {
        const int T = cT[j];
        rec_box[(long)bc * P + j] = cbox[j];
        rec_score[(long)bc * P + j] = ((cS[j] / (float)T) * (float)min(T, V)) / fv;
    }
    if (tid == 0) counts[bc] = ncl;
}

__global__ __launch_bounds__(256) void wbf_emit_kernel(const int *__restrict__ counts, const f32x4 *__restrict__ rec_box, const float *__restrict__ rec_score,
                                                       float *__restrict__ out_conf, float *__restrict__ out_xy_min, float *__restrict__ out_xy_max,
                                                       int *__restrict__ rows, int *flags, int C, int P, int R) {
    __shared__ int scan[256];
    __shared__ int soff[257];
    const int b = blockIdx.x, tid = threadIdx.x;
    float *oc = out_conf + (long)b * R * C, *omn = out_xy_min + (long)b * R * 2, *omx = out_xy_max + (long)b * R * 2;
    for (long i = tid; i < (long)R * C; i += 256) oc[i] = 0.0f;
    for (long i = tid; i < (long)R * 2; i += 256) { omn[i] = 0.0f; omx[i] = 0.0f; }
    __syncthreads();                                         // (the rows below overwrite zeros of other threads)
    long done = 0;                                           // clusters of the classes before c0
    for (int c0 = 0; c0 < C; c0 += 256) {
        scan[tid] = c0 + tid < C ? counts[(long)b * C + c0 + tid] : 0;
        __syncthreads();
        for (int d = 1; d < 256; d <<= 1) {
            const int v = tid >= d ? scan[tid - d] : 0;
            __syncthreads();
            scan[tid] += v;
            __syncthreads();
        }
        soff[tid + 1] = scan[tid];
        if (tid == 0) soff[0] = 0;
        __syncthreads();
        const int total = soff[256];
        for (int i = tid; i < total && done + i < R; i += 256) {
            int lo = 0, hi = 256;                            // the last u with soff[u] <= i: classes without clusters are skipped
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (soff[mid] <= i) lo = mid; else hi = mid;
            }
            const long rec = ((long)b * C + c0 + lo) * P + (i - soff[lo]);
            const long r = done + i;
            const f32x4 bx = rec_box[rec];
            oc[r * C + c0 + lo] = rec_score[rec];
            omn[r * 2] = bx[0]; omn[r * 2 + 1] = bx[1];
            omx[r * 2] = bx[2]; omx[r * 2 + 1] = bx[3];
        }
        done += total;
        __syncthreads();
    }
    if (tid == 0) {
        rows[b] = (int)(done < R ? done : R);
        if (done > R) atomicOr(flags, YOLO2_WBF_FLAG_ROWS);
    }
}

static size_t wbf_counts_bytes(int B, int C) { return (sizeof(int) * (size_t)B * C + 15) & ~(size_t)15; }

extern "C" size_t yolo2_wbf_workspace_bytes(int B, int C, int max_per_class) {
    if (B <= 0 || C <= 0 || max_per_class <= 0) return 0;
    return wbf_counts_bytes(B, C) + 20 * (size_t)B * C * max_per_class;
}

extern "C" int yolo2_tta_gather(const float *conf, const float *xy_min, const float *xy_max, float *out_conf, float *out_xy_min, float *out_xy_max,
                                int B, int N, int C, int M, int offset, float sx, float sy, float cell_w0, int flip, void *stream) {
    Y2_CHECK_ARG(conf && xy_min && xy_max && out_conf && out_xy_min && out_xy_max);
    Y2_CHECK_ARG(B > 0 && N > 0 && C > 0 && M >= 1 && M <= 32768);
    Y2_CHECK_ARG(offset >= 0 && N <= M && offset <= M - N);
    Y2_CHECK_ARG(isfinite(sx) && isfinite(sy) && isfinite(cell_w0));
    Y2_CHECK_ARG(flip == 0 || flip == 1);
    const long total = (long)B * N * C;
    Y2_CHECK_ARG((total + 255) / 256 <= 0x7fffffffL);
    tta_gather_kernel<<<(unsigned)((total + 255) / 256), 256, 0, (hipStream_t)stream>>>(conf, xy_min, xy_max, out_conf, out_xy_min, out_xy_max, total, N, C, M,
                                                                                        offset, sx, sy, cell_w0, flip);
    Y2_CHECK_LAUNCH();
    return YOLO2_OK;
}

extern "C" int yolo2_wbf(const float *conf, const float *xy_min, const float *xy_max, float *out_conf, float *out_xy_min, float *out_xy_max, int *rows,
                         int *flags, void *ws, int B, int M, int C, int V, int max_per_class, int R, float threshold, float fuse_iou, void *stream) {
    Y2_CHECK_ARG(conf && xy_min && xy_max && out_conf && out_xy_min && out_xy_max && rows && flags && ws);
    Y2_CHECK_ARG(B > 0 && M >= 1 && M <= 32768 && C >= 1);
    Y2_CHECK_ARG((long)B * C <= 0x7fffffffL);
    Y2_CHECK_ARG(threshold >= 0.0f);                         // (false for NaN)
    Y2_CHECK_ARG(isfinite(fuse_iou));
    Y2_CHECK_ARG(V >= 1 && max_per_class >= 1 && max_per_class <= 1024 && R >= 1);
    hipStream_t st = (hipStream_t)stream;
    const int P = max_per_class, Kcap = M < YOLO2_WBF_MAX_CANDIDATES ? M : YOLO2_WBF_MAX_CANDIDATES;
    int NP = 2;
    while (NP < Kcap) NP <<= 1;
    int *counts = (int *)ws;
    f32x4 *rec_box = (f32x4 *)((char *)ws + wbf_counts_bytes(B, C));
    float *rec_score = (float *)(rec_box + (size_t)B * C * P);
    const size_t lds = 8 * (size_t)NP + 16 * (size_t)Kcap + 40 * (size_t)P + 8 * 8 + 4 * 4;       // <= 139344 bytes
    if (lds > 64 * 1024) {
        // the attribute is per device and per kernel: remember what it has been raised to, as yolo2_soft_nms does
        static std::atomic<size_t> lds_set[64];
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = -1;
        if (dev < 0 || lds > lds_set[dev].load(std::memory_order_relaxed)) {
            if (hipFuncSetAttribute((const void *)wbf_fuse_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
                yolo2_set_error("wbf: cannot reserve %zu bytes of LDS", lds);
                return YOLO2_E_LAUNCH;
            }
            if (dev >= 0) lds_set[dev].store(lds, std::memory_order_relaxed);
        }
    }
    wbf_fuse_kernel<<<B * C, 256, lds, st>>>(conf, xy_min, xy_max, counts, rec_box, rec_score, flags, M, C, V, P, Kcap, NP, threshold, fuse_iou);
    Y2_CHECK_LAUNCH();
    wbf_emit_kernel<<<B, 256, 0, st>>>(counts, rec_box, rec_score, out_conf, out_xy_min, out_xy_max, rows, flags, C, P, R);
    Y2_CHECK_LAUNCH();
    return YOLO2_OK;
}
