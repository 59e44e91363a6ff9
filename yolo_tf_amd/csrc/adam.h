// The Adam update of one parameter, shared by optim.hip and filter_prep.hip.
#pragma once
#include "common.h"

__device__ __forceinline__ void adam_one(float &w, float g, float &m, float &v, float alpha, float omb1, float omb2, float eps, float gs) {
    // no FMA contraction: the update is inlined into several kernels (adam_kernel, adam_filter_prep_kernel) whose results must agree bit
    // for bit, and separate multiplies / adds are what the oracle (and TF's Eigen expression) evaluates
#pragma clang fp contract(off)
    const float gi = g * gs;
    const float mi = m + (gi - m) * omb1;
    const float vi = v + (gi * gi - v) * omb2;
    m = mi;
    v = vi;
    w = w - (mi * alpha) / (sqrtf(vi) + eps);
}
