// What the one-channel kernels share (vip_gray.hip: bilateral and joint bilateral;
// vip_gray_adaptive.hip: adaptive bilateral; vip_joint_f32.hip: joint bilateral of an f32 source,
// a guide and a float plane; vip_upsample.hip: joint bilateral upsampling, the same two planes at
// low resolution): the plane word of a pixel, the guide and tile loaders and the register-staged
// tile prefetch (Guide4, GrayGroup, F32Group, C1Prefetch), the byte-exact stores, the forms
// of a tap's colour-LUT index (GraySad, GrayAdaptiveDist; F32Sad is vip_joint_f32.hip's) and, for
// the radius-specialised kernels, the tap loop of one tile row (gray_row_taps) and the
// one-plane kernels' row around it (gray_tile_row). The runtime-radius kernels' tile geometry
// and launch are vip_rt.hpp's, the radius dispatch and the persistent launch vip_launch.hpp's
// (dispatch_radius, launch_c1_tiles).
#pragma once

#include "vip_rt.hpp"

namespace vip {

// GUIDE: 0 plain, 1 gray guide, 3 interleaved 3-channel guide
template <int GUIDE>
struct GrayWord {
    static_assert(GUIDE == 0 || GUIDE == 1 || GUIDE == 3, "guide channels");
    static constexpr uint32_t MASK = GUIDE == 3 ? 0xffffffu : 0xffu;   // the guide's bytes
    static constexpr int SHIFT = GUIDE == 3 ? 24 : (GUIDE == 1 ? 8 : 0);  // the source's byte
    static constexpr int ENTRIES = GUIDE == 3 ? 768 : 256;              // colour-LUT entries d can reach
    static constexpr bool TWO = false;     // one plane: the word holds guide and source
    static constexpr int LUT_SHIFT = 7;    // LUT byte address: d << 7 | 4 * copy (kGrayCopies)
    __device__ __forceinline__ static uint32_t guide(uint32_t w) { return GUIDE == 0 ? w : (w & MASK); }
    __device__ __forceinline__ static float source(uint32_t w) { return (float)((w >> SHIFT) & 0xffu); }
};
constexpr int kGrayCopies = 32;
static_assert(kGrayCopies * 4 == 1 << GrayWord<0>::LUT_SHIFT, "LUT address: d << 7");

// LutStage for 8 copies (LutStage takes 16 or 32): word d * 8 + c = color[d], two uint4 stores per
// entry (vip_joint_conf.hip and vip_joint_f32c.hip, where 16 copies leave LDS for 4 waves only)
template <int NT, int ENTRIES>
struct LutStage8 {
    static constexpr int N = ENTRIES * 2;  // uint4 stores
    static constexpr int K = (N + NT - 1) / NT;
    uint32_t v[K];
    __device__ __forceinline__ void load(const float* color) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int q = (int)threadIdx.x + k * NT;
            if (N % NT == 0 || q < N) v[k] = __float_as_uint(color[q >> 1]);
        }
    }
    __device__ __forceinline__ void store(uint32_t* lut) const {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int q = (int)threadIdx.x + k * NT;
            if (N % NT == 0 || q < N) *reinterpret_cast<uint4*>(lut + 4 * q) = make_uint4(v[k], v[k], v[k], v[k]);
        }
    }
};

// 4 gray pixels of one image row from column x (columns clamped to the image), pixel k in
// byte k: one dword load when the group is interior and the row is dword aligned.
__device__ __forceinline__ uint32_t load_gray4(const uint8_t* row, int x, int width, int aligned) {
    if (aligned && x >= 0 && x + 3 < width) return *reinterpret_cast<const uint32_t*>(row + x);
    return (uint32_t)row[clampi(x + 0, 0, width - 1)] | ((uint32_t)row[clampi(x + 1, 0, width - 1)] << 8) |
           ((uint32_t)row[clampi(x + 2, 0, width - 1)] << 16) | ((uint32_t)row[clampi(x + 3, 0, width - 1)] << 24);
}

// The guide's 4 pixels of one image row from column x (columns clamped to the image) as its 1
// (g0) or 3 dwords: dword loads when the group is interior and the row is dword aligned.
template <int GUIDE>
struct Guide4 {
    uint32_t g0, g1, g2;

    __device__ __forceinline__ void load(const uint8_t* row, int x, int width, int aligned) {
        g0 = g1 = g2 = 0u;
        if constexpr (GUIDE == 1) g0 = load_gray4(row, x, width, aligned);
        if constexpr (GUIDE == 3) {
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
};

// One 4-pixel group as loaded from HBM (the source dword and the guide's 1 or 3 dwords),
// and as the 4 plane words it becomes.
template <int GUIDE>
struct GrayGroup {
    static constexpr bool TWO = false;  // one plane
    uint32_t s;
    Guide4<GUIDE> g;

    __device__ __forceinline__ void load(const uint8_t* src, long long src_pitch, const uint8_t* guide,
                                         long long guide_pitch, int sy, int x, int width, int aligned) {
        s = load_gray4(src + (long long)sy * src_pitch, x, width, aligned);
        g.load(guide + (long long)sy * guide_pitch, x, width, aligned);
    }
    __device__ __forceinline__ uint4 words() const {
        uint4 r;
        if constexpr (GUIDE == 0) {
            r.x = s & 0xffu;
            r.y = (s >> 8) & 0xffu;
            r.z = (s >> 16) & 0xffu;
            r.w = s >> 24;
        } else if constexpr (GUIDE == 1) {
            r.x = (g.g0 & 0xffu) | ((s & 0xffu) << 8);
            r.y = ((g.g0 >> 8) & 0xffu) | (s & 0xff00u);
            r.z = ((g.g0 >> 16) & 0xffu) | ((s >> 8) & 0xff00u);
            r.w = (g.g0 >> 24) | ((s >> 16) & 0xff00u);
        } else {
            const uint4 u = unpack_rgb4(g.g0, g.g1, g.g2);
            r.x = u.x | (s << 24);
            r.y = u.y | ((s & 0xff00u) << 16);
            r.z = u.z | ((s & 0xff0000u) << 8);
            r.w = u.w | (s & 0xff000000u);
        }
        return r;
    }
};

// 4 pixels of one image row from column x (columns clamped to the image): the guide's 1 or 3
// dwords and the source's 4 floats, as loaded from HBM, and as the plane words they become
// (words(): the guide plane's; source_words(): the float plane's).
template <int GUIDE>
struct F32Group {
    static constexpr bool TWO = true;
    Guide4<GUIDE> g;
    float4 f;

    __device__ __forceinline__ void load(const uint8_t* src, long long src_pitch, const uint8_t* guide,
                                         long long guide_pitch, int sy, int x, int width, int aligned) {
        const bool interior = x >= 0 && x + 3 < width;
        const float* frow = reinterpret_cast<const float*>(src + (long long)sy * src_pitch);
        if ((aligned & kF32SrcVec) && interior) {
            f = *reinterpret_cast<const float4*>(frow + x);
        } else {
            f.x = frow[clampi(x + 0, 0, width - 1)];
            f.y = frow[clampi(x + 1, 0, width - 1)];
            f.z = frow[clampi(x + 2, 0, width - 1)];
            f.w = frow[clampi(x + 3, 0, width - 1)];
        }
        // with or without `interior` the flag means the same (Guide4 tests the columns itself); each
        // guide form gets the spelling that compiles to the code it had (profiles/c1_shared_isa.txt)
        const int gwords = aligned & kF32GuideWords;
        g.load(guide + (long long)sy * guide_pitch, x, width, GUIDE == 3 ? (gwords && interior) : gwords);
    }
    __device__ __forceinline__ uint4 words() const {
        if constexpr (GUIDE == 1)
            return make_uint4(g.g0 & 0xffu, (g.g0 >> 8) & 0xffu, (g.g0 >> 16) & 0xffu, g.g0 >> 24);
        return unpack_rgb4(g.g0, g.g1, g.g2);
    }
    __device__ __forceinline__ uint4 source_words() const {
        return make_uint4(__float_as_uint(f.x), __float_as_uint(f.y), __float_as_uint(f.z), __float_as_uint(f.w));
    }
};

// Write P float outputs of row oy from column x (a multiple of P): 16-byte stores where dst
// allows them (dst_aligned: base and pitch are 16-byte aligned) and the outputs are all inside
// the row, single dwords otherwise; never a byte at column >= width or row >= out_rows.
template <int P, class A>
__device__ __forceinline__ void store_f32(const A& a, int oy, int x, const float (&o)[P]) {
    static_assert(P == 4 || P == 8, "outputs per thread");
    if (oy >= a.out_rows || x >= a.width) return;
    float* p = reinterpret_cast<float*>(a.dst + (long long)oy * a.dst_pitch) + x;
    if (a.dst_aligned && x + P <= a.width) {
#pragma unroll
        for (int q = 0; q < P / 4; ++q)
            reinterpret_cast<float4*>(p)[q] = make_float4(o[4 * q], o[4 * q + 1], o[4 * q + 2], o[4 * q + 3]);
        return;
    }
#pragma unroll
    for (int i = 0; i < P; ++i)
        if (x + i < a.width) p[i] = o[i];
}

// A third plane is a policy of the GROUP (the tile loaders) and of the DIST (the tap loop): a
// type that declares THREE = true (vip_joint_conf.hip's ConfGroup and ConfSad: a confidence
// plane beside the guide and source planes). Every other type has two planes at most, and the
// third-plane text below is discarded for it at compile time.
template <class T>
constexpr bool has_third_plane() {
    if constexpr (requires { T::THREE; })
        return T::THREE;
    else
        return false;
}

// Register-staged prefetch of one tile's plane or planes (TilePrefetch's one-channel form), in
// GROUPs of 4 pixels (GrayGroup: one plane; F32Group: a guide and a float
// plane; a three-plane GROUP: a confidence plane as well): issue() starts the HBM loads of source rows [ty0 + src_row0 - R, +ROWS) x columns
// [tx0 - L, tx0 + TW + L), rows clamped to [row_lo, row_hi), columns to [0, width); commit()
// writes the plane words: the GROUP's words() and, with GROUP::TWO, its source_words() to fplane
// (a three-plane GROUP: its conf_words() to cplane too; such a GROUP loads from the kernel's own
// argument struct, which holds the third array).
template <int R, int ROWS, int NT, int P, class GROUP>
struct C1Prefetch {
    using G = Geom<R, P, 16>;
    static constexpr int NG = ROWS * G::GROUPS;
    static constexpr int K = (NG + NT - 1) / NT;
    static constexpr bool THREE = has_third_plane<GROUP>();
    GROUP raw[K];

    template <class ARGS>
    __device__ __forceinline__ void issue(const ARGS& a, int tx0, int ty0) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int g = (int)threadIdx.x + k * NT;
            if (NG % NT != 0 && k == K - 1 && g >= NG) continue;
            const int r = g / G::GROUPS;
            const int gc = g - r * G::GROUPS;
            const int sy = clampi(ty0 + a.src_row0 - R + r, a.row_lo, a.row_hi - 1);
            if constexpr (THREE)
                raw[k].load(a, sy, tx0 - G::L + 4 * gc);
            else
                raw[k].load(a.src, a.src_pitch, a.guide, a.guide_pitch, sy, tx0 - G::L + 4 * gc, a.width, a.aligned);
        }
    }
    __device__ __forceinline__ void commit(uint32_t* plane, uint32_t* fplane = nullptr,
                                           uint32_t* cplane = nullptr) const {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int g = (int)threadIdx.x + k * NT;
            if (NG % NT != 0 && k == K - 1 && g >= NG) continue;
            const int r = g / G::GROUPS;
            const int gc = g - r * G::GROUPS;
            *reinterpret_cast<uint4*>(plane + r * G::S + 4 * gc) = raw[k].words();
            if constexpr (GROUP::TWO) *reinterpret_cast<uint4*>(fplane + r * G::S + 4 * gc) = raw[k].source_words();
            if constexpr (THREE) *reinterpret_cast<uint4*>(cplane + r * G::S + 4 * gc) = raw[k].conf_words();
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

// ---- a tap's colour-LUT index d, in two forms. Each is a plane-word reading (guide(w): what
// the index is formed from; source(w): the neighbour's float) plus index(g, nf, i): d of the
// neighbour with guide word g and float nf against the thread's output i. TWO: the source has
// a plane of its own and source() reads that plane's word; LUT_SHIFT: the LUT's byte address is
// d << LUT_SHIFT | 4 * copy. (A third form, F32Sad, is vip_joint_f32.hip's.)
constexpr int kGrayAdaEntries = 512;  // the adaptive form's int(dist) <= 510

// bilateral / joint bilateral: the sum of absolute byte differences of the guide words
template <int GUIDE, int P>
struct GraySad : GrayWord<GUIDE> {
    uint32_t ctr[P];  // the outputs' centre guide words
    __device__ __forceinline__ uint32_t index(uint32_t g, float, int i) const {
        return __builtin_amdgcn_sad_u8(g, ctr[i], 0u);
    }
};
// adaptive: |(n - c) - o| on the plain plane word, c the centre and o = c - box mean
template <int P>
struct GrayAdaptiveDist {
    static constexpr int ENTRIES = kGrayAdaEntries;
    static constexpr bool TWO = false;
    static constexpr int LUT_SHIFT = 7;
    float cf[P], of[P];
    __device__ __forceinline__ static uint32_t guide(uint32_t w) { return w; }
    __device__ __forceinline__ static float source(uint32_t w) { return (float)w; }
    // (float)(n - c) == f_n - f_c exactly; int(dist) <= 510
    __device__ __forceinline__ uint32_t index(uint32_t, float nf, int i) const {
        return (uint32_t)__builtin_fabsf((nf - cf[i]) - of[i]);
    }
};

// The third plane's words of one tile row beside a RowStream, read chunk by chunk with it (a
// RowStream of the one plane); nothing at all without a third plane.
template <int C0, int NC, bool THREE>
struct ThirdRow {
    __device__ __forceinline__ ThirdRow(const uint32_t*, int) {}
    __device__ __forceinline__ void load(int) {}
};
template <int C0, int NC>
struct ThirdRow<C0, NC, true> {
    RowStream<C0, NC, false> row;
    __device__ __forceinline__ ThirdRow(const uint32_t* cplane, int row_off) : row(cplane, cplane, row_off) {}
    __device__ __forceinline__ void load(int q) { row.load(q); }
    __device__ __forceinline__ float word(int k) const { return __uint_as_float(row.guide(k)); }
};

// The tap loop of one tile row (row_taps' one-accumulator form): neighbour column j serves
// output i at kx = j - L - i; per output the taps run in ascending kx. fplane: the source's
// plane when DIST::TWO, else not read (the callers pass plane again). cplane: read only by a
// three-plane DIST (has_third_plane): the plane of the neighbour's confidence c_n, and the
// weight sum is then sumk = fma(c_n, w, sumk) (sumk + c_n * w without FMA) instead of sumk + w.
template <int HW, int L, int C0, int NC, bool FMA, int P, class DIST>
__device__ __forceinline__ void gray_row_taps(const uint32_t* plane, const uint32_t* fplane, int row_off,
                                              const float (&wsv)[HW + 1], const char* lut, uint32_t lane4,
                                              const DIST& dist, float (&s)[P], float (&sk)[P],
                                              const uint32_t* cplane = nullptr) {
    constexpr int D = kPipeDepth, NB = D + 1;
    constexpr int J0 = L - HW, J1 = L + P - 1 + HW;
    constexpr int LA = D + kRowLookahead;
    constexpr bool THREE = has_third_plane<DIST>();
    static_assert(J0 >= 4 * C0 && J1 < 4 * (C0 + NC), "row chunk range");
    auto chunk = [](int j) constexpr { return (j - 4 * C0) >> 2; };
    constexpr int PRE = chunk(J0 + LA < J1 ? J0 + LA : J1);
    RowStream<C0, NC, DIST::TWO> row(plane, fplane, row_off);
    ThirdRow<C0, NC, THREE> crow(cplane, row_off);
#pragma unroll
    for (int q = 0; q <= PRE; ++q) row.load(q), crow.load(q);
    float wc[NB][P], nf[NB];
    [[maybe_unused]] float nc[NB];
    auto issue = [&](int j) {
        const uint32_t g = DIST::guide(row.guide(j - 4 * C0));
        const int b = (j - J0) % NB;
        nf[b] = DIST::source(row.source(j - 4 * C0));
        if constexpr (THREE) nc[b] = crow.word(j - 4 * C0);
#pragma unroll
        for (int i = 0; i < P; ++i) {
            const int kx = j - L - i;
            if (kx < -HW || kx > HW) continue;
            const uint32_t d = dist.index(g, nf[b], i);
            wc[b][i] = *reinterpret_cast<const float*>(lut + ((d << DIST::LUT_SHIFT) | lane4));
        }
    };
#pragma unroll
    for (int j = J0; j < J0 + D && j <= J1; ++j) issue(j);
#pragma unroll
    for (int j = J0; j <= J1; ++j) {
        if (j + LA <= J1 && ((j + LA) & 3) == 0 && chunk(j + LA) > PRE) row.load(chunk(j + LA)), crow.load(chunk(j + LA));
        if (j + D <= J1) issue(j + D);
        const int b = (j - J0) % NB;
#pragma unroll
        for (int i = 0; i < P; ++i) {
            const int kx = j - L - i;
            if (kx < -HW || kx > HW) continue;
            const float w = wc[b][i] * wsv[kx < 0 ? -kx : kx];
            if constexpr (FMA)
                s[i] = __builtin_fmaf(nf[b], w, s[i]);
            else
                s[i] = s[i] + nf[b] * w;
            if constexpr (!THREE)
                sk[i] = sk[i] + w;
            else if constexpr (FMA)
                sk[i] = __builtin_fmaf(nc[b], w, sk[i]);
            else
                sk[i] = sk[i] + nc[b] * w;
        }
        __builtin_amdgcn_sched_barrier(0);
    }
}

// Tile row ky of the persistent one-plane kernels, what for_each_row<R, true> runs per row: the
// wave's priority band, the row's spatial weights (uniform: scalar loads), the taps, and the
// accumulators pinned at the row's end (fence_accumulators). row_off: the plane word of the
// thread's row ky, column tx * P. (joint_f32_kernel keeps a row body of its own: through this
// function its 12-wave instantiations allocate registers differently.)
template <int R, int HW, int L, bool FMA, int P, class DIST>
__device__ __forceinline__ void gray_tile_row(const StencilArgs& a, int ky, const uint32_t* plane, int row_off,
                                              const char* lut, uint32_t lane4, const DIST& dist, float (&s)[P],
                                              float (&sk)[P]) {
    const int aky = ky < 0 ? -ky : ky;
    set_progress_priority((ky + R) * 4 / (2 * R + 1));
    const float* const ws = a.ws + aky * kWsStride;
    constexpr int C0 = (L - HW) / 4, C1 = (L + P - 1 + HW) / 4;
    constexpr int NC = C1 - C0 + 1;
    float wsv[HW + 1];
#pragma unroll
    for (int k = 0; k <= HW; ++k) wsv[k] = ws[k];
    gray_row_taps<HW, L, C0, NC, FMA, P>(plane, plane, row_off, wsv, lut, lane4, dist, s, sk);
#pragma unroll
    for (int i = 0; i < P; ++i) __asm__ volatile("" : "+v"(s[i]), "+v"(sk[i]));
}

}  // namespace vip
