// The wide-store epilogue of the implicit-GEMM kernels (conv_igemm.hip, conv_pp.hip, conv_s4.hip, conv_d1.hip), device code: each wave
// rounds its sub-tile into a private, padded LDS image, takes the forward BN statistics from the rounded values on the way, reads the
// image back row-major (16 bytes per lane and store), optionally adds the producer layer's BN + leaky backward sums (Y2BnBwd), and
// publishes either result into the [2][Y2_BN_PART_ROWS][C] partial rows.  The arithmetic and its order live here, once; WHEN the loads
// are issued, how far the loops are unrolled and where the waits sit is scheduling and stays with each kernel.
#pragma once
#include "conv_shared.h"
#include "bn_leaky.h"

// ---- partial rows.  The rows are indexed by a row id the kernel derives from its plan (conv_shared.h: Y2IgemmPlan, Y2P_ / Y2S_ / D1_STAT_ROWS*);
// the host counts the same ids and, when they exceed the rows the consumer reads, wraps them (Y2BnBwd::stat_mask_inv).  When they fit,
// every (row, filter) has exactly one writer: plain stores into the zeroed row, bitwise-reproducible sums -- and the f32 atomics of the
// 13x13 stages (each a fabric round trip) were 10 us of a 77 us launch (profiles/r02_igemm_ablation.txt).  Wrapped rows keep the atomic
// adds: same-address f32 atomics serialise at ~0.1 us each (12 us of the 52 x 52 BN-backward launch's 52, profiles/r06_pp_bn_epilogue.txt),
// which is why wave rows meet in LDS first wherever the LDS plan has room (y2_wave_rows_meet).
struct Y2PartRows {
    float *part;
    int Nf, stat_mask_inv;
    bool unique;      // one writer per (row, filter): the host found a row for every row id (no wrap)
    static __device__ __forceinline__ Y2PartRows of(float *part, int Nf, int stat_mask_inv) { return Y2PartRows{part, Nf, stat_mask_inv, stat_mask_inv == 0}; }
    __device__ __forceinline__ int slot(int row_id) const { return row_id & ((Y2_BN_PART_ROWS - 1) ^ stat_mask_inv); }
    // one filter per lane: the forward statistics sum(y - shift) [plane 0], sum((y - shift)^2) [plane 1]
    __device__ __forceinline__ void publish(int row_id, int n, float s1, float s2) const {
        const int s = slot(row_id);
        float *p1 = part + (long)s * Nf + n, *p2 = part + (long)(Y2_BN_PART_ROWS + s) * Nf + n;
        if (unique) { *p1 = s1; *p2 = s2; }
        else { unsafeAtomicAdd(p1, s1); unsafeAtomicAdd(p2, s2); }
    }
    // VEC consecutive filters per lane: the BN-backward sums
    template <int VEC> __device__ __forceinline__ void publish(int row_id, int nb, const float (&ps)[2][VEC]) const {
        const int s = slot(row_id);
        float *p1 = part + (long)s * Nf + nb, *p2 = part + (long)(Y2_BN_PART_ROWS + s) * Nf + nb;
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            if (unique) { p1[k] = ps[0][k]; p2[k] = ps[1][k]; }
            else { unsafeAtomicAdd(p1 + k, ps[0][k]); unsafeAtomicAdd(p2 + k, ps[1][k]); }
        }
    }
};

// ---- BN + leaky backward sums of the producer layer: the per-channel constants and running sums of the VEC filters a lane keeps in every
// store iteration (64 % WCPR == 0)
template <typename T> struct Y2BnBwdLane {
    static constexpr int VEC = 16 / (int)sizeof(T);
    float cmu[VEC], cinv[VEC], cga[VEC], cbt[VEC], ps[2][VEC];
    __device__ __forceinline__ void load(const Y2BnBwd &bz, int nb) {
#pragma unroll
        for (int k = 0; k < VEC; k += 4) {
            const f32x4 a = *reinterpret_cast<const f32x4 *>(bz.mean + nb + k), b = *reinterpret_cast<const f32x4 *>(bz.var + nb + k);
            const f32x4 c = *reinterpret_cast<const f32x4 *>(bz.gamma + nb + k), d = *reinterpret_cast<const f32x4 *>(bz.beta + nb + k);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                cmu[k + q] = a[q];
                cinv[k + q] = bn_inv_std(b[q], bz.eps);
                cga[k + q] = c[q];
                cbt[k + q] = d[q];
                ps[0][k + q] = ps[1][k + q] = 0.f;
            }
        }
    }
    // bn_leaky.h bn_leaky_bwd, spelled out (the helper perturbs these MFMA kernels' schedules), on the rounded gradient d just stored and the producer's stored y
    __device__ __forceinline__ void add(const Y2BnBwd &bz, const Vec16<T> &y, const Vec16<T> &d) {
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            const float xh = (y.get(k) - cmu[k]) * cinv[k];
            const float z = (y.get(k) - cmu[k]) * (cinv[k] * cga[k]) + cbt[k];
            const float g = z >= 0.f ? d.get(k) : bz.alpha * d.get(k);
            ps[0][k] += g * xh;
            ps[1][k] += g;
        }
    }
    // the lanes that share a channel chunk (lane % WCPR) meet on the VALU: common.h y2_lane_group_sum
    template <int WCPR> __device__ __forceinline__ void lane_group_sum() {
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            ps[0][k] = y2_lane_group_sum<WCPR>(ps[0][k]);
            ps[1][k] = y2_lane_group_sum<WCPR>(ps[1][k]);
        }
    }
};
template <typename T> __device__ __forceinline__ Vec16<T> y2_as_vec16(f32x4 v) {
    Vec16<T> d;
    d.v = __builtin_bit_cast(decltype(d.v), v);
    return d;
}

// The WGM wave rows of a tile hold sums of the SAME channels: they meet in LDS (`red`: NW * WCPR * 2 * VEC floats) and the tile leaves ONE
// partial row per filter -- a WGM-th of the adds and of the row ids competing for the partial rows.  Every wave calls it (one barrier);
// afterwards the lanes with `summer` (wave row 0, lane < WCPR, filter in range) hold the tile's sums, wave rows added in index order.
template <int WGM, int WGN, int WCPR, int VEC>
__device__ __forceinline__ void y2_wave_rows_meet(float *red, int wave, int wn, int lane, bool summer, float (&ps)[2][VEC]) {
    if (lane < WCPR) {
#pragma unroll
        for (int k = 0; k < VEC; ++k) { red[(wave * WCPR + lane) * 2 * VEC + k] = ps[0][k]; red[(wave * WCPR + lane) * 2 * VEC + VEC + k] = ps[1][k]; }
    }
    __syncthreads();
    if (summer) {
#pragma unroll
        for (int r = 1; r < WGM; ++r)
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                ps[0][k] += red[((r * WGN + wn) * WCPR + lane) * 2 * VEC + k];
                ps[1][k] += red[((r * WGN + wn) * WCPR + lane) * 2 * VEC + VEC + k];
            }
    }
}

// ---- staging: accumulator column j, 32-row blocks [I0, I1), rounded into this wave's LDS image (+ the forward statistics of the rounded
// values, published under row_id).  C/D layout of the 32x32 MFMA: col = lane & 31, row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5).
// act (leaky ReLU of a BN-folded inference layer) and tail (the last pixel tile: rows >= M stay out of the sums; mrow0 = pixel of image
// row 0) are tested inside the 16-element loop: two to three VALU per element each (~10 % of the ~7 us a tile's epilogue takes) unless
// the caller passes std::true_type / std::false_type and chooses among the specialised copies with ONE uniform branch.
template <int I0, int I1, int WSTRIDE, typename T, int TM, int TN, typename ActTag, typename TailTag>
__device__ __forceinline__ void y2_stage_column(const f32x16 (&acc)[TM][TN], int j, unsigned char *wreg, int lane, float bv, float act_alpha, ActTag act,
                                                TailTag tail, int mrow0, int M, bool stats, float sh, const Y2PartRows &rows, int row_id, int n, bool n_ok) {
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = I0; i < I1; ++i) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = i * 32 + 4 * (lane >> 5) + (r & 3) + 8 * (r >> 2);
            float v = acc[i][j][r] + bv;
            if (act) v = fmaxf(v, act_alpha * v);
            const T o = (T)v;
            *reinterpret_cast<T *>(wreg + row * WSTRIDE + (j * 32 + (lane & 31)) * (int)sizeof(T)) = o;
            if (stats && (!tail || mrow0 + row < M)) {
                const float d = (float)o - sh;
                s1 += d;
                s2 += d * d;
            }
        }
    }
    if (stats) {      // lanes l and l ^ 32 hold the same column
        s1 += __shfl_xor(s1, 32, 64);
        s2 += __shfl_xor(s2, 32, 64);
        if (lane < 32 && n_ok) rows.publish(row_id, n, s1, s2);
    }
}

// ---- store loop body: position id = it * 64 + lane of the rows [row0, ...) of this wave's image -> one 16-byte store of VEC consecutive
// filters of one pixel (mrow0 = pixel of image row 0, ncol0 = filter of image column 0), + the BN-backward sums of the stored values (y: the
// producer's y at the same place).  after_read runs between the LDS read and the store: where a kernel issues its next group of y loads.
struct Y2NoHook { __device__ __forceinline__ void operator()() const {} };
template <int WSTRIDE, int WCPR, typename T, typename AfterRead = Y2NoHook>
__device__ __forceinline__ void y2_store_chunk(const unsigned char *wreg, int id, int row0, T *O, int ldo, int mrow0, int M, int ncol0, int Nf, bool bstats,
                                               Y2BnBwdLane<T> &bw, const Y2BnBwd &bz, const Vec16<T> &y, AfterRead after_read = AfterRead{}) {
    const int row = row0 + id / WCPR, ch = id % WCPR;
    const int m = mrow0 + row;
    const int n = ncol0 + ch * Y2BnBwdLane<T>::VEC;
    const f32x4 v = *reinterpret_cast<const f32x4 *>(wreg + row * WSTRIDE + ch * 16);
    after_read();
    if (m < M && n < Nf) {
        *reinterpret_cast<f32x4 *>(O + (long)m * ldo + n) = v;
        if (bstats) bw.add(bz, y, y2_as_vec16<T>(v));
    }
}
