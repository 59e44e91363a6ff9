// The scalar arithmetic the head kernels share (head.hip: loss and decode; distill.hip), so that the f32 bound derived for one
// (tests/head_cases.py) holds for the other.  The softmax of both is max -> sum of expf(z - max) -> expf(z - max) / sum, serial in the lane.
#pragma once

__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + expf(-x)); }
