// What the fused texture guide stages share (vip_texture.hip: the 3-channel stage and the
// fused iteration; vip_gray_texture.hip: the one-channel stage): the guide tile and workgroup
// per radius, the per-thread run lengths of the phases, and the packed sliding-window helpers.
#pragma once

#include "vip_exact.hpp"
#include "vip_launch.hpp"
#include "vip_stencil.hpp"

namespace vip {

// Guide tile (TW x TH outputs) and workgroup size, per radius. The phases run one
// work item per thread where the counts allow it: 4 vertically adjacent blur
// positions per pass-2 run, 4 vertically adjacent guide outputs per guide run, so a
// (TW + 2R) x (TH + 2R) blur region of up to 1024 pass-2 runs fills 1024 threads once.
// 92 x 36 at R = 2 (k = 5, C4): 96 x 40 blur positions = 960 pass-2 runs (1.159 per
// output), 828 guide runs, 2160 = 60 tile rows exactly, 75 KiB of LDS -> two 16-wave
// workgroups per CU. Measured per 4K iteration (guide stage + JBF, round 2,
// profiles/r02_variants.txt): 64 x 16 / 256 threads 158.4-159.7 us, 124 x 28 / 1024
// 150.3-150.7 us (60 x 60: 157.5, 28 x 124: 154.2, 252 x 12: 177.0, 60 x 28 / 512: 165.3);
// round 5, per C4 frame on one stream, interleaved on one box
// (profiles/r05_gf_tiles_{a,b,c}.txt): 92 x 36 656.1-661.0 us against 124 x 28
// 661.7-667.2 (96 x 36 668-671, 124 x 24 673, 108 x 32 678-680, 80 x 40 697, 80 x 44 692,
// 60 x 60 693).
struct GfTile { int tw, th, nt; };
// Tiles per radius for R > 2 (texture ksize 6..24; the reference's default ksize 9 is R = 4).
// Round 6, kernel-stamped 4K launches interleaved on one box against the 64 x 16 / 256-thread
// tile (profiles/r06_guide_tiles_big_r_ab{,2}.txt), per launch.
constexpr GfTile gf_tile(int R) {
    if (R <= 2) return GfTile{92, 36, 1024};
    switch (R) {
        case 3: return GfTile{92, 32, 1024};  // 110.7 -> 91.1 us (1.33 blur positions per output against 1.64)
        case 4: return GfTile{92, 32, 1024};  // VGPRs capped at 64 (10 spilled): 134.4 -> 110.5 us
        case 5: return GfTile{92, 32, 1024};  // uncapped: 216.6 -> 192.3 us (capped spills 37: 211.5)
        case 6: return GfTile{64, 16, 256};   // 60 x 36: 300.5 us, capped 261.6, against 263.8
        case 7: return GfTile{60, 36, 1024};  // capped (49 spilled): 446.7 -> 394.5 us
        default: return GfTile{64, 16, 256};
    }
}
// minimum waves per SIMD the guide-stage kernel of radius R is compiled for (1: no cap; 8 caps
// the VGPRs at 64, two 1024-thread workgroups per CU: the capped tiles of gf_tile)
constexpr int gf_min_waves(int R) { return R == 4 || R == 7 ? 8 : 1; }
constexpr int kGfH1 = 8;   // pass 1: horizontally adjacent window aggregates per thread
constexpr int kGfV2 = 4;   // pass 2: vertically adjacent blur positions per thread
constexpr int kGfRun = 4;  // guide: vertically adjacent outputs per thread

constexpr int cmax(int a, int b) { return a > b ? a : b; }

typedef short gf_s16x2 __attribute__((ext_vector_type(2)));
typedef unsigned short gf_u16x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ uint32_t pk_max_u16(uint32_t a, uint32_t b) {
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(gf_u16x2, a),
                                                                  __builtin_bit_cast(gf_u16x2, b)));
}

// N sliding maxima (any associative, idempotent op) of K consecutive terms: blocks of
// K, suffix scans inside a block and prefix scans into the next, window j =
// op(suffix[j], prefix[j + K - 1]) (van Herk / Gil-Werman).
template <int N, int K, class T, class Op>
__device__ __forceinline__ void win_op(const T (&x)[N + K - 1], T (&o)[N], Op op) {
    constexpr int M = N + K - 1;
    T suf[M], pre[M];
#pragma unroll
    for (int b0 = 0; b0 < M; b0 += K) {
        const int b1 = (b0 + K < M ? b0 + K : M) - 1;
        suf[b1] = x[b1];
#pragma unroll
        for (int t = b1 - 1; t >= b0; --t) suf[t] = op(x[t], suf[t + 1]);
        pre[b0] = x[b0];
#pragma unroll
        for (int t = b0 + 1; t <= b1; ++t) pre[t] = op(pre[t - 1], x[t]);
    }
#pragma unroll
    for (int j = 0; j < N; ++j) o[j] = (j % K == 0) ? suf[j] : op(suf[j], pre[j + K - 1]);
}

}  // namespace vip
