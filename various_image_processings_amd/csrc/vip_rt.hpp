// What the runtime-radius kernels share (vip_stencil_rt.hip: stencil_rt_kernel; vip_gray.hip:
// gray_rt_kernel; vip_gray_adaptive.hip: gray_adaptive_rt_kernel): the 64 x 64 tile geometry,
// the constant-address-space qualifier of their uniform tables and the host side of a launch.
// Each kernel keeps its own LUT fill, plane fill and row loop: moved into shared functions they
// compile to other scalar code in every kernel (runtime-radius kernel).
#pragma once

#include "vip_launch.hpp"
#include "vip_stencil.hpp"

namespace vip {

constexpr int kRtP = 4;           // outputs per thread
constexpr int kRtTW = 16 * kRtP;  // tile width in pixels
constexpr int kRtWaves = 16;      // 64 tile rows

// LDS words of one tile plane: (64 + 2R) rows x S words, + a zeroed pad when the apron is
// narrower than the one-block over-read of the last row (R = 0 only)
__host__ __device__ constexpr int rt_plane_words(int R, int L, int S) {
    return (kRtWaves * 4 + 2 * R) * S + (L < 4 ? 8 : 0);
}
// S = 64 or 128: the 16-lane groups of a ds_read_b128 hit disjoint banks
__host__ __device__ constexpr int rt_stride(int L) { return kRtTW + 2 * L <= 64 ? 64 : 128; }

// The spatial table and the half-widths are read-only for the whole launch: read them
// through the constant address space so the uniform loads become scalar loads.
#define kconst __attribute__((address_space(4)))

// The launcher's part of RtArgs: apron L, plane stride S and the tile columns.
inline int rt_prepare(RtArgs& a) {
    if (a.R < 0 || a.R > kRtMaxRadius) return VIP_ERR_UNSUPPORTED_KSIZE;
    a.L = round_up(a.R, 4);
    a.S = rt_stride(a.L);
    a.tiles_x = (a.width + kRtTW - 1) / kRtTW;
    return 0;
}

// One workgroup per tile of a prepared launch, with lds_bytes of dynamic LDS (a radius whose
// planes and LUT do not fit the CU is unsupported).
template <auto KERN>
int launch_rt_tiles(const RtArgs& a, long long lds_bytes, hipStream_t stream) {
    if (lds_bytes > kLdsBudget) return VIP_ERR_UNSUPPORTED_KSIZE;
    if (const int rc = ensure_lds<KERN>(kLdsBudget)) return rc;
    note_launch(reinterpret_cast<const void*>(KERN));
    const int tiles_y = (a.out_rows + kRtWaves * 4 - 1) / (kRtWaves * 4);
    const long long tiles = (long long)a.tiles_x * tiles_y;
    if (tiles == 0) return 0;
    if (tiles > 0x7fffffffLL) return VIP_ERR_INVALID_ARGUMENT;
    launch(KERN, dim3((unsigned)tiles), dim3(kRtWaves * 64), (uint32_t)lds_bytes, stream, a);
    return (int)hipGetLastError();
}

}  // namespace vip
