// soft_exp: the exponential of the Soft-NMS Gaussian weight (soft_nms.hip), written so that NumPy float32 can restate it operation for
// operation (tests/soft_nms_ref.py): only f32 + - x, rintf and integer operations, no FMA, no library exp.
//   n = rint(x * log2e);  r = (x - n * LN2_HI) - n * LN2_LO  (Cody-Waite: LN2_HI has 9 significant bits, n * LN2_HI is exact);
//   p = the degree-7 Taylor polynomial of e^r by Horner's rule, every product and every sum rounded on its own;  result = p * 2^n, 2^n built in
//   the exponent bits.
// Valid for -65 <= x <= 0 (n >= -94: 2^n is a normal number, the scaling is exact).  soft_exp(+-0) == 1.0f exactly (n = 0, r = 0, p = 1).
// |soft_exp(x) / exp(x) - 1| <= 2^-21 on [-65, 0]: the remainder after degree 7 is below 6e-9 (|r| <= 0.3466), the rest is a handful of
// roundings (tests/test_soft_nms_cpu.py sweeps it against f64).
// The including translation unit must be built with FP contraction off (-ffp-contract=off); the pragma below covers this header's own code.
#pragma once
#pragma clang fp contract(off)

#if defined(__HIPCC__)
#define SOFT_EXP_FN __host__ __device__ __forceinline__
#else
#define SOFT_EXP_FN static inline
#endif

SOFT_EXP_FN float soft_exp(float x) {
    const float LOG2E = 1.44269504f, LN2_HI = 0.693359375f, LN2_LO = -2.12194440e-4f;
    const float n = rintf(x * LOG2E);
    float r = x - n * LN2_HI;
    r = r - n * LN2_LO;
    float p = 1.98412698e-4f;              // 1/5040
    p = p * r + 1.38888889e-3f;            // 1/720
    p = p * r + 8.33333333e-3f;            // 1/120
    p = p * r + 4.16666667e-2f;            // 1/24
    p = p * r + 1.66666667e-1f;            // 1/6
    p = p * r + 0.5f;
    p = p * r + 1.0f;
    p = p * r + 1.0f;
    const unsigned bits = (unsigned)((int)n + 127) << 23;
    return p * __builtin_bit_cast(float, bits);
}
