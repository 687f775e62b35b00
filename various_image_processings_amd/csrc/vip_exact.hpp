// Exact-arithmetic device helpers (correctly rounded divisions, square root, exp), each
// checked by microbench/div_check.hip: the texture stages use them, the stencil epilogue
// (vip_stencil.hpp finish_outputs) recip_exact and div_by_sumk.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

namespace vip {

// Correctly rounded (float)s / d for an integer box sum s and the constant d = k^2
// (or 3): q0 = s*rd, one fma residual, one fma correction. Equal to the IEEE quotient
// for every s in [0, k^2 * 255], k <= 31 -- checked exhaustively in
// tests/test_oracle.py::test_constant_division_is_exact (rd = RN(1/d)).
__device__ __forceinline__ float div_exact(uint32_t s, float d, float rd) {
    const float f = (float)s;
    const float q0 = f * rd;
    return __builtin_fmaf(__builtin_fmaf(-q0, d, f), rd, q0);
}

// RN(sqrt(x)) for x = 0 or x in [1, 2^24) (the texture gradient's integer sums of
// squares): the hardware v_sqrt_f32 result s and one neighbour check each way -- the
// refinement LLVM's correctly rounded sqrtf expansion applies, without its denormal
// scaling and special-value handling, which these arguments never need. 9 VALU
// instead of 17; microbench/div_check.hip verifies it against sqrtf for EVERY integer
// in [0, 2^20) (the gradient sums stay below 6 * 255^2 = 390150).
__device__ __forceinline__ float sqrt_int_exact(float x) {
    const float s = __builtin_amdgcn_sqrtf(x);
    const float sm = __uint_as_float(__float_as_uint(s) - 1u);
    const float s1 = __builtin_fmaf(-sm, s, x) <= 0.f ? sm : s;
    const float sp = __uint_as_float(__float_as_uint(s) + 1u);
    return __builtin_fmaf(-sp, s, x) > 0.f ? sp : s1;
}

// 2^(j/64), j = 0..63, correctly rounded to double (staged into LDS by the kernels that
// call exp_tab_f32; internal linkage, one copy per translation unit).
static __constant__ double kExp2Tab64[64] = {
#include "vip_exp_tab64.inc"
};

// (float)exp((double)x) for float x in [0, 32) -- the texture guide's alpha argument
// sigma_alpha * (rtv - rtv_min) lies in [0, 255 / (5 ksize)] -- in 14 double ops:
// x = (k/64) ln2 + r with |r| <= ln2/128 (two-part Cody-Waite; k < 2^12, so k * HI is
// exact), exp(r) - 1 by its degree-5 Taylor polynomial (truncation < 2^-54), times
// 2^(k mod 64 / 64) from `etab` (kExp2Tab64 in LDS) and 2^(k / 64). microbench/div_check
// compares it with (float)exp((double)x) for EVERY float in [0, 32).
__device__ __forceinline__ float exp_tab_f32(float xf, const double* etab) {
    const double x = (double)xf;
    const double kd = __builtin_rint(x * 0x1.71547652b82fep+6);  // 64 / ln2
    const int k = (int)kd;
    double r = __builtin_fma(-kd, 0x1.62e42fefa3000p-7, x);       // ln2/64, 12 low bits clear
    r = __builtin_fma(-kd, 0x1.3de6af278ece6p-48, r);             // ln2/64 - HI
    double q = __builtin_fma(r, 1.0 / 120, 1.0 / 24);
    q = __builtin_fma(r, q, 1.0 / 6);
    q = __builtin_fma(r, q, 0.5);
    const double p = __builtin_fma(r * r, q, r);                  // exp(r) - 1
    const double t = etab[k & 63];
    return (float)__builtin_ldexp(__builtin_fma(t, p, t), k >> 6);
}

// clampi((int)v, 0, 255) written into byte `sel` of `word`: floor (the int conversion's
// truncation for v >= 0, and below 0 either way) then v_cvt_pk_u8_f32, whose float->u8
// conversion saturates (an integral input, so its rounding is moot) and packs in the same
// instruction. microbench/div_check compares it with the clamp for every float |v| < 2048.
__device__ __forceinline__ uint32_t pack_u8_clamped(float v, uint32_t sel, uint32_t word) {
    return __builtin_amdgcn_cvt_pk_u8_f32(__builtin_floorf(v), sel, word);
}

// RN(1/k) for k in [1, 2^38): hardware rcp (1 ulp) + one Newton step. Verified
// exhaustively over every float of that range by microbench/div_check.hip.
__device__ __forceinline__ float recip_exact(float k) {
    const float y0 = __builtin_amdgcn_rcpf(k);
    return __builtin_fmaf(__builtin_fmaf(-k, y0, 1.0f), y0, y0);
}

// (float)(n / d) with the IEEE double quotient: the texture guide stage's rtv (CUDA profile,
// src/bilateral_texture_filter_impl.cu:99-101), n = (double)num in [0, 2^18), d =
// (double)msum + 1e-9 in [1e-9, 2^20): no scaling is ever needed. Two Newton steps from
// v_rcp_f64 give r = 1/d to within a few 2^-53 (the first two steps of the compiler's own
// f64 division), so q = RN(n r) is within 4 double ulps of n/d, and RN_f(q) equals
// RN_f(RN_d(n/d)) unless n/d lies within that distance of a float rounding midpoint --
// which q's 29 low mantissa bits show (midpoint: 2^28). Those lanes (about 2^-23 of them)
// take the IEEE division. 7 f64 ops + 3 integer ops against the division's 11 f64 ops.
// microbench/div_check compares it with (float)(n / d) on 2^30 inputs, half of them at
// midpoints. The guide stage itself keeps the IEEE division (exact and measured 0.4 % slower
// per C4 frame there); div_check is its only caller.
__device__ __forceinline__ float rtv_quotient(double n, double d) {
    const double r0 = __builtin_amdgcn_rcp(d);
    double e = __builtin_fma(-d, r0, 1.0);
    double r = __builtin_fma(r0, e, r0);
    e = __builtin_fma(-d, r, 1.0);
    r = __builtin_fma(r, e, r);
    const double q = n * r;
    const uint32_t lo = (uint32_t)__builtin_bit_cast(unsigned long long, q);
    if (__builtin_expect(((lo & 0x1fffffffu) - (0x10000000u - 64u)) < 128u, 0)) return (float)(n / d);
    return (float)q;
}

// RN(s / k) given y = RN(1/k) (Markstein): q0 = RN(s y) is within 1 ulp of s/k, the
// residual s - k q0 is exact under fma, and one correction rounds correctly. Needs
// no over/underflow: s in [0, 255 k], k in [1, 1024). Cross-checked on 2^30 random
// and near-midpoint quotients by microbench/div_check.hip.
__device__ __forceinline__ float div_by_sumk(float s, float k, float y) {
    const float q0 = s * y;
    return __builtin_fmaf(__builtin_fmaf(-k, q0, s), y, q0);
}

}  // namespace vip
