// Batch norm + leaky ReLU (+ 2x2 max pool) element arithmetic, device code: the expressions and their order live here, once.  The kernels of
// bn.hip / bn_stats.hip keep their own loops, loads and schedule and call these for the values wherever that leaves their code as it was
// (profiles/elementwise_split.md lists the sites where it does not: those spell the same expression out, with a comment).
#pragma once
#include "common.h"

__device__ __forceinline__ float bn_inv_std(float var, float eps) { return 1.0f / sqrtf(var + eps); }

// ---- forward value
__device__ __forceinline__ float bn_leaky(float y, float mu, float sc, float bt, float alpha) {
    const float z = (y - mu) * sc + bt;
    return fmaxf(z, alpha * z);
}

// ---- backward term: g = d * leaky'(z), xh = the normalised y;  dgamma = sum g * xh, dbeta = sum g
struct BnBwdTerm { float g, xh; };
__device__ __forceinline__ BnBwdTerm bn_leaky_bwd(float y, float d, float mu, float inv, float ga, float bt, float alpha) {
    const float xh = (y - mu) * inv;
    const float z = (y - mu) * (inv * ga) + bt;
    const float g = z >= 0.f ? d : alpha * d;
    return BnBwdTerm{g, xh};
}
// dy from the term; dgm = dgamma / M, dbm = dbeta / M
__device__ __forceinline__ float bn_bwd_apply(const BnBwdTerm &t, float inv, float ga, float dgm, float dbm) {
    return (ga * inv) * (t.g - dbm - t.xh * dgm);
}

// ---- the 2x2 window: positions 0..3 in scan order (0,0),(0,1),(1,0),(1,1), one arg-max byte per element
template <int N> struct IdxPack;      // N arg-max bytes as one integer
template <> struct IdxPack<8> { typedef unsigned long long type; };
template <> struct IdxPack<4> { typedef unsigned int type; };
template <int N> __device__ __forceinline__ typename IdxPack<N>::type idx_pack_byte(int arg, int j) { return (typename IdxPack<N>::type)arg << (8 * j); }
template <typename P> __device__ __forceinline__ int idx_pack_get(P pack, int j) { return (int)((pack >> (8 * j)) & 3); }

struct PoolRow {   // pooled pixel r -> element offset of the window's top-left input pixel
    int OH, OW, H, W, C;
    __device__ PoolRow(int H_, int W_, int C_) : OH(H_ / 2), OW(W_ / 2), H(H_), W(W_), C(C_) {}
    __device__ long base(long r) const {
        const int ow = (int)(r % OW);
        const long t = r / OW;
        const int oh = (int)(t % OH);
        const long b = t / OH;
        return ((b * H + oh * 2) * W + ow * 2) * C;
    }
};

// an activation ROUNDED to T (= what an unfused producer stores and a separate pool reads); the maximum of a window's four rounded activations
// and (returned) the position of the first maximum
template <typename T> __device__ __forceinline__ float pool_round(float x) { return (float)(T)x; }
__device__ __forceinline__ int pool_first_max(const float (&a)[4], float &m) {
    m = fmaxf(fmaxf(a[0], a[1]), fmaxf(a[2], a[3]));
    return a[0] == m ? 0 : a[1] == m ? 1 : a[2] == m ? 2 : 3;
}
// the inverse: the pooled gradient d as seen from position k of a window whose arg-max is `arg`
__device__ __forceinline__ float pool_route(int arg, int k, float d) { return arg == k ? d : 0.f; }

// ---- the moving-average update (assign_moving_average: moving -= (1 - decay) * (moving - batch), omd = 1 - decay)
__device__ __forceinline__ float bn_ema(float m, float x, float omd) { return m - (m - x) * omd; }
