// Shared device/host helpers for the MI355X (gfx950) bilateral-filter family.
// Replaces src/device_utilities.cuh (clamp) and src/host_utilities.hpp
// (CUDASafeCall) of the reference with a status-returning HIP layer.
#pragma once

#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>
#include <cstdlib>

#include "vip.h"

namespace vip {

// Reference: src/device_utilities.cuh:5-10.
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// static_cast<uint8_t>(v) for v in [0, 256); v_cvt_i32_f32 maps NaN to 0.
__device__ __forceinline__ uint32_t f2u8(float v) { return (uint32_t)(int)v & 0xffu; }

// Round a launch-time size up to a multiple.
constexpr int round_up(int v, int m) { return (v + m - 1) / m * m; }

// Circle half-width of row ky for a disc of radius R: the largest |kx| with
// kx^2 + ky^2 <= R^2 (src/bilateral_filter_impl.cu:222-231 masks the square LUT
// with the same test, so taps outside it carry an exact zero weight).
__host__ __device__ constexpr int isqrt_floor(int v) {
    int r = 0;
    while ((r + 1) * (r + 1) <= v) ++r;
    return r;
}
__host__ __device__ constexpr int circle_hw(int R, int ky) { return isqrt_floor(R * R - ky * ky); }

// Distinct squared tap distances v = kx^2 + ky^2 <= R^2 of the disc (0 <= kx, ky <= R),
// ranked in ascending order: the folded colour x space LUT of the bilateral kernel
// holds one table per distinct v.
__host__ __device__ constexpr bool is_disc_r2(int R, int v) {
    for (int a = 0; a <= R; ++a)
        for (int b = 0; b <= R; ++b)
            if (a * a + b * b == v) return true;
    return false;
}
__host__ __device__ constexpr int disc_r2_rank(int R, int v) {  // distinct disc values below v
    int n = 0;
    for (int u = 0; u < v && u <= R * R; ++u) n += is_disc_r2(R, u) ? 1 : 0;
    return n;
}
__host__ __device__ constexpr int disc_r2_count(int R) { return disc_r2_rank(R, R * R + 1); }

}  // namespace vip

// Record the first error of a call; launch errors come back through
// hipGetLastError (the reference printed them and carried on,
// src/host_utilities.hpp:9-13; the C ABI returns them instead).
#define VIP_HIP_CHECK(expr)                                  \
    do {                                                     \
        hipError_t _e = (expr);                              \
        if (_e != hipSuccess) return (int)_e;                \
    } while (0)
