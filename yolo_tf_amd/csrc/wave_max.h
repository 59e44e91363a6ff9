// The maximum of a 64-bit key over a wave, shared by the kernels whose serial loops select by a strict total order (soft_nms.hip's pick,
// tta.hip's best cluster): the key decides alone, so the shape of the reduction cannot matter.
#pragma once

typedef unsigned long long u64;

__device__ __forceinline__ u64 snms_u64(unsigned lo, unsigned hi) { return ((u64)hi << 32) | lo; }
__device__ __forceinline__ u64 snms_max(u64 a, u64 b) { return a > b ? a : b; }
#if defined(__HIP_DEVICE_COMPILE__)
// maximum of a 64-bit key over the wave, left in every lane: rotations inside the 16-lane rows (DPP), then the row pairs and the halves
// (permlane swaps of a value with its copy: see y2_lane_group_sum_f64 of common.h, whose exchanges these are)
template <int CTRL> __device__ __forceinline__ u64 snms_dpp(u64 v) {
    return snms_u64((unsigned)__builtin_amdgcn_mov_dpp((int)(unsigned)v, CTRL, 0xF, 0xF, true), (unsigned)__builtin_amdgcn_mov_dpp((int)(unsigned)(v >> 32), CTRL, 0xF, 0xF, true));
}
__device__ __forceinline__ u64 snms_wave_max(u64 v) {
    v = snms_max(v, snms_dpp<0x121>(v));      // row_ror:1
    v = snms_max(v, snms_dpp<0x122>(v));      // row_ror:2
    v = snms_max(v, snms_dpp<0x124>(v));      // row_ror:4
    v = snms_max(v, snms_dpp<0x128>(v));      // row_ror:8
    {
        unsigned lo = (unsigned)v, hi = (unsigned)(v >> 32), lo2 = lo, hi2 = hi;
        asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1\n\tv_permlane16_swap_b32 %2, %3\n\ts_nop 1" : "+v"(lo), "+v"(lo2), "+v"(hi), "+v"(hi2));
        v = snms_max(snms_u64(lo, hi), snms_u64(lo2, hi2));
    }
    {
        unsigned lo = (unsigned)v, hi = (unsigned)(v >> 32), lo2 = lo, hi2 = hi;
        asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1\n\tv_permlane32_swap_b32 %2, %3\n\ts_nop 1" : "+v"(lo), "+v"(lo2), "+v"(hi), "+v"(hi2));
        v = snms_max(snms_u64(lo, hi), snms_u64(lo2, hi2));
    }
    return v;
}
#else
__device__ inline u64 snms_wave_max(u64 v) { return v; }      // (host pass of a __global__ body)
#endif
