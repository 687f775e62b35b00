// What the single-channel (8-bit gray) kernels share (vip_gray.hip: bilateral and joint
// bilateral; vip_gray_adaptive.hip: adaptive bilateral): the plane word of a pixel, the tile
// loaders, the byte-exact store and the runtime-radius kernels' tile geometry.
#pragma once

#include "vip_launch.hpp"
#include "vip_stencil.hpp"

namespace vip {

// GUIDE: 0 plain, 1 gray guide, 3 interleaved 3-channel guide
template <int GUIDE>
struct GrayWord {
    static_assert(GUIDE == 0 || GUIDE == 1 || GUIDE == 3, "guide channels");
    static constexpr uint32_t MASK = GUIDE == 3 ? 0xffffffu : 0xffu;   // the guide's bytes
    static constexpr int SHIFT = GUIDE == 3 ? 24 : (GUIDE == 1 ? 8 : 0);  // the source's byte
    static constexpr int ENTRIES = GUIDE == 3 ? 768 : 256;              // colour-LUT entries d can reach
    __device__ __forceinline__ static uint32_t guide(uint32_t w) { return GUIDE == 0 ? w : (w & MASK); }
    __device__ __forceinline__ static float source(uint32_t w) { return (float)((w >> SHIFT) & 0xffu); }
};
constexpr int kGrayCopies = 32;

// 4 gray pixels of one image row from column x (columns clamped to the image), pixel k in
// byte k: one dword load when the group is interior and the row is dword aligned.
__device__ __forceinline__ uint32_t load_gray4(const uint8_t* row, int x, int width, int aligned) {
    if (aligned && x >= 0 && x + 3 < width) return *reinterpret_cast<const uint32_t*>(row + x);
    return (uint32_t)row[clampi(x + 0, 0, width - 1)] | ((uint32_t)row[clampi(x + 1, 0, width - 1)] << 8) |
           ((uint32_t)row[clampi(x + 2, 0, width - 1)] << 16) | ((uint32_t)row[clampi(x + 3, 0, width - 1)] << 24);
}

// One 4-pixel group as loaded from HBM (the source dword and the guide's 1 or 3 dwords),
// and as the 4 plane words it becomes.
template <int GUIDE>
struct GrayGroup {
    uint32_t s, g0, g1, g2;

    __device__ __forceinline__ void load(const uint8_t* src, long long src_pitch, const uint8_t* guide,
                                         long long guide_pitch, int sy, int x, int width, int aligned) {
        s = load_gray4(src + (long long)sy * src_pitch, x, width, aligned);
        g0 = g1 = g2 = 0u;
        if constexpr (GUIDE == 1) g0 = load_gray4(guide + (long long)sy * guide_pitch, x, width, aligned);
        if constexpr (GUIDE == 3) {
            const uint8_t* row = guide + (long long)sy * guide_pitch;
            if (aligned && x >= 0 && x + 3 < width) {
                const uint32_t* w = reinterpret_cast<const uint32_t*>(row + 3 * x);
                g0 = w[0];
                g1 = w[1];
                g2 = w[2];
            } else {
                const uint32_t q0 = load_rgb(row, clampi(x + 0, 0, width - 1));
                const uint32_t q1 = load_rgb(row, clampi(x + 1, 0, width - 1));
                const uint32_t q2 = load_rgb(row, clampi(x + 2, 0, width - 1));
                const uint32_t q3 = load_rgb(row, clampi(x + 3, 0, width - 1));
                g0 = q0 | (q1 << 24);
                g1 = (q1 >> 8) | (q2 << 16);
                g2 = (q2 >> 16) | (q3 << 8);
            }
        }
    }

    __device__ __forceinline__ uint4 words() const {
        uint4 r;
        if constexpr (GUIDE == 0) {
            r.x = s & 0xffu;
            r.y = (s >> 8) & 0xffu;
            r.z = (s >> 16) & 0xffu;
            r.w = s >> 24;
        } else if constexpr (GUIDE == 1) {
            r.x = (g0 & 0xffu) | ((s & 0xffu) << 8);
            r.y = ((g0 >> 8) & 0xffu) | (s & 0xff00u);
            r.z = ((g0 >> 16) & 0xffu) | ((s >> 8) & 0xff00u);
            r.w = (g0 >> 24) | ((s >> 16) & 0xff00u);
        } else {
            const uint4 u = unpack_rgb4(g0, g1, g2);
            r.x = u.x | (s << 24);
            r.y = u.y | ((s & 0xff00u) << 16);
            r.z = u.z | ((s & 0xff0000u) << 8);
            r.w = u.w | (s & 0xff000000u);
        }
        return r;
    }
};

// Register-staged prefetch of one tile plane (TilePrefetch's gray form): issue() starts the
// HBM loads of source rows [ty0 + src_row0 - R, +ROWS) x columns [tx0 - L, tx0 + TW + L),
// rows clamped to [row_lo, row_hi), columns to [0, width); commit() writes the plane words.
template <int R, int ROWS, int NT, int P, int GUIDE>
struct GrayPrefetch {
    using G = Geom<R, P, 16>;
    static constexpr int NG = ROWS * G::GROUPS;
    static constexpr int K = (NG + NT - 1) / NT;
    GrayGroup<GUIDE> raw[K];

    __device__ __forceinline__ void issue(const StencilArgs& a, int tx0, int ty0) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int g = (int)threadIdx.x + k * NT;
            if (NG % NT != 0 && k == K - 1 && g >= NG) continue;
            const int r = g / G::GROUPS;
            const int gc = g - r * G::GROUPS;
            const int sy = clampi(ty0 + a.src_row0 - R + r, a.row_lo, a.row_hi - 1);
            raw[k].load(a.src, a.src_pitch, a.guide, a.guide_pitch, sy, tx0 - G::L + 4 * gc, a.width, a.aligned);
        }
    }
    __device__ __forceinline__ void commit(uint32_t* plane) const {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int g = (int)threadIdx.x + k * NT;
            if (NG % NT != 0 && k == K - 1 && g >= NG) continue;
            const int r = g / G::GROUPS;
            const int gc = g - r * G::GROUPS;
            *reinterpret_cast<uint4*>(plane + r * G::S + 4 * gc) = raw[k].words();
        }
    }
};

// Write P gray outputs of row oy from column x: one word store where dst allows it
// (dst_aligned: base and pitch are P-byte aligned) and the outputs are all inside the row,
// single bytes otherwise; never a byte at column >= width or row >= out_rows.
template <int P, class A>
__device__ __forceinline__ void store_gray(const A& a, int oy, int x, const uint32_t (&o)[P]) {
    static_assert(P == 4 || P == 8, "outputs per thread");
    if (oy >= a.out_rows || x >= a.width) return;
    uint8_t* p = a.dst + (long long)oy * a.dst_pitch + x;
    if (a.dst_aligned && x + P <= a.width) {
        const uint32_t w0 = o[0] | (o[1] << 8) | (o[2] << 16) | (o[3] << 24);
        if constexpr (P == 8) {
            const uint32_t w1 = o[4] | (o[5] << 8) | (o[6] << 16) | (o[7] << 24);
            *reinterpret_cast<uint2*>(p) = make_uint2(w0, w1);
        } else {
            *reinterpret_cast<uint32_t*>(p) = w0;
        }
        return;
    }
#pragma unroll
    for (int i = 0; i < P; ++i)
        if (x + i < a.width) p[i] = (uint8_t)o[i];
}

// ---- the runtime-radius kernels' tile
constexpr int kGrayRtP = 4;                // outputs per thread
constexpr int kGrayRtTW = 16 * kGrayRtP;   // tile width in pixels
constexpr int kGrayRtWaves = 16;           // 64 tile rows

// LDS words of the tile plane: (64 + 2R) rows x S words, + a zeroed pad when the apron is
// narrower than the one-block over-read of the last row (R = 0 only)
__host__ __device__ constexpr int gray_rt_plane_words(int R, int L, int S) {
    return (kGrayRtWaves * 4 + 2 * R) * S + (L < 4 ? 8 : 0);
}
// S = 64 or 128: the 16-lane groups of a ds_read_b128 hit disjoint banks
__host__ __device__ constexpr int gray_rt_stride(int L) { return kGrayRtTW + 2 * L <= 64 ? 64 : 128; }

// The spatial table and the half-widths are read-only for the whole launch: read them
// through the constant address space so the uniform loads become scalar loads.
#define kconst __attribute__((address_space(4)))

}  // namespace vip
