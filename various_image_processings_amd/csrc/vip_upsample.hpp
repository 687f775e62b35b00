// What the joint-bilateral-upsampling kernels share (vip_upsample.hip: one channel;
// vip_upsample_f32c.hpp: 2..4 interleaved channels): the tile geometry in low-resolution cells,
// the guide words and the colour-LUT address, and the reader of a thread's window of a plane row.
#pragma once

#include "vip_gray.hpp"

namespace vip {

constexpr int kUpP = 8;            // outputs per thread
constexpr int kUpTW = 16 * kUpP;   // tile width in output pixels
constexpr int kUpWaves = 16;
constexpr int kUpTH = 64;          // tile height: 4 rows per wave
constexpr int kUpCopies = 32;      // interleaved copies of each colour-LUT entry
constexpr int kUpLutShift = 7;     // LUT byte address: d << 7 | 4 * copy

// WAVES: waves per workgroup, 4 output rows each (the one-channel kernel: kUpWaves everywhere)
template <int R, int S, int WAVES = kUpWaves>
struct UpGeom {
    static_assert(R >= 0 && R <= kUpMaxRadius && (S == 2 || S == 4 || S == 8), "radius, scale");
    static constexpr int TH = WAVES * 4;                  // tile height in output pixels
    static constexpr int CW = kUpTW / S, CH = TH / S;     // the tile in cells
    static constexpr int L = round_up(R, 4);              // left/right apron in cells
    static constexpr int GROUPS = (CW + 2 * L) / 4;       // 4-cell groups per plane row
    static constexpr int ROWS = CH + 2 * R;
    static constexpr int NG = ROWS * GROUPS;
    static constexpr int NC = kUpP / S;                   // cells under a thread's outputs
    static constexpr int NW = NC + 2 * R;                 // cells a thread reads per tap row
    static constexpr int NAX = S * R + S / 2;             // spatial table: NAX x NAX
    // Plane row stride in words. A wave reads the windows of 4 plane rows at once, lane group q
    // at row q, lane tx at column tx * NC (+ a constant):
    //   S = 2  the window is read as (2L + 4) / 4 aligned ds_read_b128 from column 4 tx (OFF
    //          words before the first cell used); 16 lanes read 64 contiguous words of a row:
    //          LS = 0 (mod 64) keeps the lane groups of a b128 read on distinct banks
    //   S = 4  ds_read_b32, 32 lanes = 2 rows x even columns 0..30: LS odd
    //   S = 8  ds_read_b32, 32 lanes = 2 rows x columns 0..15: LS = 16 (mod 32)
    static constexpr int LS = S == 2 ? round_up(CW + 2 * L, 64)
                                     : (S == 4 ? CW + 2 * L + 1 : round_up(CW + 2 * L - 16, 32) + 16);
    static constexpr int OFF = S == 2 ? L - R : 0;
    static constexpr int NWL = S == 2 ? 2 * L + 4 : NW;   // words a thread loads per tap row and plane
    static_assert(LS >= CW + 2 * L && OFF + NW <= NWL, "plane row");
    static_assert(NG <= WAVES * 64, "one plane group per thread");
    static_assert(WAVES % S == 0 && (WAVES / S) * 4 * S == TH, "a wave's rows share their phase");
};
static_assert(UpGeom<0, 2>::TH == kUpTH, "the one-channel tile");
template <int GUIDE>
constexpr int up_lut_entries() {
    static_assert(GUIDE == 1 || GUIDE == 3, "guide channels");
    return GUIDE == 3 ? 768 : 256;
}
template <int R, int S, int GUIDE>
constexpr int up_lds_bytes() {
    return 4 * (up_lut_entries<GUIDE>() * kUpCopies + 2 * UpGeom<R, S>::ROWS * UpGeom<R, S>::LS);
}

// 4 guide pixels as loaded (Guide4) -> their 4 guide words, of the low-resolution plane and of the
// outputs' centres alike: B | G << 8 | R << 16 of a 3-channel guide, G << 7 of a gray one.
template <int GUIDE>
__device__ __forceinline__ uint4 up_guide_words(const Guide4<GUIDE>& g) {
    if constexpr (GUIDE == 1)
        return make_uint4((g.g0 & 0xffu) << kUpLutShift, ((g.g0 >> 8) & 0xffu) << kUpLutShift,
                          ((g.g0 >> 16) & 0xffu) << kUpLutShift, (g.g0 >> 24) << kUpLutShift);
    return unpack_rgb4(g.g0, g.g1, g.g2);
}
// LDS byte address of a tap's colour weight: d << 7 | 4 * copy (lanec), d the distance of the
// two guide words. A gray guide's words are the 16-bit values G << 7, whose absolute difference
// is d << 7 already: v_sad_u16 forms it and adds lanec in one instruction; a 3-channel guide's d
// is the v_sad_u8 sum of its three byte differences, shifted after.
template <int GUIDE>
__device__ __forceinline__ uint32_t up_lut_address(uint32_t g, uint32_t c, uint32_t lanec) {
    if constexpr (GUIDE == 1) return __builtin_amdgcn_sad_u16(g, c, lanec);
    return (__builtin_amdgcn_sad_u8(g, c, 0u) << kUpLutShift) | lanec;
}

// N words of a plane row from p: whole ds_read_b128 (VEC: p is 16-byte aligned, N a multiple
// of 4; volatile keeps each a full b128, as RowStream's) or single words
template <int N, bool VEC>
__device__ __forceinline__ void up_load_window(const uint32_t* p, uint32_t (&w)[N]) {
    if constexpr (VEC) {
        static_assert(N % 4 == 0, "whole chunks");
        typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
        typedef __attribute__((address_space(3))) const volatile u32x4 lds_u32x4;
        lds_u32x4* const q = (lds_u32x4*)(p);
#pragma unroll
        for (int c = 0; c < N / 4; ++c) {
            const u32x4 v = q[c];
            w[4 * c + 0] = v.x; w[4 * c + 1] = v.y; w[4 * c + 2] = v.z; w[4 * c + 3] = v.w;
        }
    } else {
#pragma unroll
        for (int k = 0; k < N; ++k) w[k] = p[k];
    }
}

}  // namespace vip
