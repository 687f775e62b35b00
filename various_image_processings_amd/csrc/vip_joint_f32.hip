// Joint bilateral filter of an f32 one-channel source under an 8-bit guide, for gfx950 (MI355X).
//
// Definition (include/vip.h, vip_joint_bilateral_run_f32): per output pixel and per tap in
// row-major order over the k x k square, w = ws[ky,kx] * wc[d], s = fmaf(f_n, w, s) (CUDA
// profile) or s + f_n * w (CPP profile), sumk += w, dst = s / sumk (IEEE binary32 division, no
// rounding to integer, no clamp), replicate border; d = |G_n - G_c| (gray guide) or
// |dB| + |dG| + |dR| (3-channel guide). Every weight and every LDS address comes from the
// guide, so the source may hold any float: s and sumk are the floats of
// vip_joint_bilateral_run_c1 when f == (float)g. The build's -O3 -ffp-contract=off leaves the
// kernels in denorm mode 3 (.amdhsa_float_denorm_mode_32 3): gradual underflow, as the definition.
//
// Two LDS planes, a guide word and a float per pixel (as the two-plane stencil_rt_kernel
// <..., JOINT>), not one 64-bit plane: a ds_read_b128 of either plane then feeds 4 neighbours
// exactly as the gray kernels' one plane does, the row strides and their bank-conflict-free
// ds_read_b128 groups (Geom::S, rt_stride) carry over unchanged, and RowStream<.., TWO> already
// reads such a pair: the guide loader, the tile prefetch and the tap loop of a tile row are the
// gray kernels' (vip_gray.hpp: Guide4, C1Prefetch on F32Group, gray_row_taps with the F32Sad
// index). A 64-bit plane would interleave guide and float in every ds_read_b128
// (2 neighbours per read) and double every row stride. The guide plane holds the bare guide
// word (G, or B | G << 8 | R << 16), so v_sad_u8 needs no mask; the float plane is the
// neighbour itself: a tap is the gray kernels' minus the byte -> float conversion per
// neighbour word, plus one more ds_read_b128 per 4 neighbours.
//
// LDS budget (kLdsBudget = 160 KiB; planes of 4 bytes per pixel each):
//   gray guide       256 x 32 LUT copies (32 KiB); 16 waves fit at every radius
//                    (R = 15: 2 x 61,664 + 32,768 = 156,096 B)
//   3-channel guide  768 x 32 copies (96 KiB) fit beside two planes at no radius with 16 waves
//                    (R = 1: 73,920 + 98,304 = 172,224 B), so the LUT holds 768 x 16 copies
//                    (48 KiB; lanes l and l + 16 share a copy: <= 2-way bank conflicts, as the
//                    joint kernels' 16-copy LUT); 16 waves fit up to R = 12 (158,976 B), 12
//                    waves beyond (R = 15: 102,336 + 49,152 = 151,488 B): pick_waves
//   The wave count is the smaller of what LDS and what the registers allow (f32_waves): 16
//   waves up to R = 12 (gray guide) or 9 (3-channel guide), 12 waves above.
//   runtime radius   the same LUTs; R = 23 (ksize 47, the joint filter's limit):
//                    2 x 56,320 + 49,152 = 161,792 B with a 3-channel guide
//
// Two kernels, as for the other filters:
//   joint_f32_kernel<R, GUIDE, FMA>   radius 1..15 a template argument; persistent workgroups
//       over 128 x 64 (16 waves) or 128 x 48 (12 waves) tiles, 8 outputs per thread, every tile
//       row straight-line code (Geom, for_each_row, RowStream), the next tile's HBM reads in
//       flight under the current tile's taps, xcd_tile's placement.
//   joint_f32_rt_kernel<GUIDE, FMA>   radius a kernel argument (0 and 16..23, or every radius
//       under VIP_PATH_RUNTIME); gray_rt_kernel's frame (vip_rt.hpp): one workgroup per 64 x 64
//       tile, 4 outputs per thread, taps in blocks of 4 with exact zero weights outside the
//       disc. A zero weight times a finite neighbour adds an exact zero, hence the finite-input
//       domain; the zero-filled pad (float 0, guide word 0) is harmless.
// StencilArgs / RtArgs are unchanged: src and dst carry the float pointers as bytes (pitches in
// bytes), `aligned` is a bit set (kF32GuideWords, kF32SrcVec) and dst_aligned means 16-byte
// aligned; the entry point (vip_capi.hip) sets them.
#include "vip_gray.hpp"

namespace vip {

constexpr int kF32P = 8;

template <int GUIDE>
struct F32Guide {
    static_assert(GUIDE == 1 || GUIDE == 3, "guide channels");
    static constexpr int ENTRIES = GUIDE == 3 ? 768 : 256;  // colour-LUT entries d can reach
    static constexpr int COPIES = GUIDE == 3 ? 16 : 32;     // interleaved copies of each entry
    static constexpr int LUT_SHIFT = COPIES == 32 ? 7 : 6;  // LUT byte address: d << LUT_SHIFT | 4 * copy
    static constexpr int LUTW = ENTRIES * COPIES;
};
// Waves per workgroup: the most whose planes fit LDS (pick_waves), and 12 from the radius on at
// which a 16-wave workgroup's 128 VGPRs no longer hold the kernel without scratch (the
// register-staged prefetch of the next tile is 5 VGPRs per 4-pixel group with a gray guide, 7
// with a 3-channel one, against the gray kernels' 2 to 4); 12 waves have 168
// (profiles/joint_f32_resources.txt).
constexpr int kF32Max16Gray = 12, kF32Max16Rgb = 9;
template <int R, int GUIDE>
constexpr int f32_waves() {
    return pick_waves<R, 2, (R <= (GUIDE == 3 ? kF32Max16Rgb : kF32Max16Gray) ? 16 : 12), F32Guide<GUIDE>::LUTW, kF32P,
                      16>();
}

// A tap's colour-LUT index (as vip_gray.hpp's GraySad): the guide plane's word is the bare
// guide, the float plane's word the neighbour's float as it stands.
template <int GUIDE, int P>
struct F32Sad : F32Guide<GUIDE> {
    static constexpr bool TWO = true;
    uint32_t ctr[P];  // the outputs' centre guide words
    __device__ __forceinline__ static uint32_t guide(uint32_t w) { return w; }
    __device__ __forceinline__ static float source(uint32_t w) { return __uint_as_float(w); }
    __device__ __forceinline__ uint32_t index(uint32_t g, float, int i) const {
        return __builtin_amdgcn_sad_u8(g, ctr[i], 0u);
    }
};

template <int R, int GUIDE, bool FMA>
__global__ __launch_bounds__((f32_waves<R, GUIDE>() * 64)) void joint_f32_kernel(const StencilArgs a) {
    using W = F32Guide<GUIDE>;
    constexpr int P = kF32P, WAVES = f32_waves<R, GUIDE>(), NT = WAVES * 64;
    using G = Geom<R, P, 16>;
    constexpr int TH = WAVES * G::RPW;
    constexpr int ROWS = TH + 2 * R;
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    uint32_t* const lut = lds;
    uint32_t* const gplane = lds + W::LUTW;
    uint32_t* const fplane = gplane + ROWS * G::S;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tx = lane & 15;
    const int ty = wave * G::RPW + (lane >> 4);
    static_assert(G::S % 4 == 0 && P % 4 == 0, "plane rows in uint4");
    const int base4 = ty * (G::S / 4) + tx * (P / 4);  // uint4 index of the thread's tile row, column tx * P
    const uint32_t lanec = (uint32_t)(lane & (W::COPIES - 1)) << 2;  // this lane's LUT copy
    const char* const lut_bytes = reinterpret_cast<const char*>(lut);

    // persistent: workgroup b filters tiles b, b + grid, ... (xcd_tile's placement)
    int tile = blockIdx.x;
    C1Prefetch<R, ROWS, NT, P, F32Group<GUIDE>> pf;
    LutStage<NT, W::ENTRIES, W::COPIES> ls;
    ls.load(a.color);
    {
        const int t = xcd_tile(tile, a.tiles_total);
        pf.issue(a, (t % a.tiles_x) * G::TW, (t / a.tiles_x) * TH);
    }
    ls.store(lut);
    pf.commit(gplane, fplane);
    __syncthreads();

    for (;;) {
        const int t = xcd_tile(tile, a.tiles_total);
        const int tx0 = (t % a.tiles_x) * G::TW, ty0 = (t / a.tiles_x) * TH;
        const int next = tile + (int)gridDim.x;
        if (next < a.tiles_total) {  // next tile's HBM reads fly under this tile's taps
            const int n = xcd_tile(next, a.tiles_total);
            pf.issue(a, (n % a.tiles_x) * G::TW, (n / a.tiles_x) * TH);
        }
        if (ty0 + wave * G::RPW < a.out_rows) {  // wave-uniform: skip rows past the band
            F32Sad<GUIDE, P> dist;
            {
                const uint4* c = reinterpret_cast<const uint4*>(gplane + (ty + R) * G::S + tx * P + G::L);
#pragma unroll
                for (int q = 0; q < P / 4; ++q) {
                    const uint4 v = c[q];
                    dist.ctr[4 * q + 0] = v.x;
                    dist.ctr[4 * q + 1] = v.y;
                    dist.ctr[4 * q + 2] = v.z;
                    dist.ctr[4 * q + 3] = v.w;
                }
            }
            float s[P], sk[P];
#pragma unroll
            for (int i = 0; i < P; ++i) s[i] = sk[i] = 0.f;

            for_each_row<R, true>([&](const int ky, auto hwc) {
                // 4 * (the thread's uint4 index + the row's constant): RowStream's row_off >> 2 then
                // folds, and every row of a plane is one base register plus a ds_read immediate
                // (as (ty + R + ky) * S + tx * P the 2 x (2R + 1) row addresses each take a VGPR)
                const int row_off = 4 * (base4 + (R + ky) * (G::S / 4));
                constexpr int HW = decltype(hwc)::value;
                const int aky = ky < 0 ? -ky : ky;
                set_progress_priority((ky + R) * 4 / (2 * R + 1));
                const float* const ws = a.ws + aky * kWsStride;
                constexpr int C0 = (G::L - HW) / 4, C1 = (G::L + P - 1 + HW) / 4;
                constexpr int NC = C1 - C0 + 1;
                float wsv[HW + 1];
#pragma unroll
                for (int k = 0; k <= HW; ++k) wsv[k] = ws[k];
                gray_row_taps<HW, G::L, C0, NC, FMA, P>(gplane, fplane, row_off, wsv, lut_bytes, lanec, dist, s, sk);
                // pin the accumulators at the row's end (fence_accumulators)
#pragma unroll
                for (int i = 0; i < P; ++i) __asm__ volatile("" : "+v"(s[i]), "+v"(sk[i]));
            });

            float o[P];
#pragma unroll
            for (int i = 0; i < P; ++i) o[i] = s[i] / sk[i];
            store_f32(a, ty0 + ty, tx0 + tx * P, o);
        }
        if (next >= a.tiles_total) break;
        __syncthreads();  // every wave is done reading this tile
        pf.commit(gplane, fplane);
        __syncthreads();
        tile = next;
    }
}

template <int GUIDE, bool FMA>
static int launch_joint_f32_dispatch(int radius, const StencilArgs& a, hipStream_t stream) {
    return dispatch_radius(radius, [&](auto rc) {
        constexpr int R = decltype(rc)::value, WAVES = f32_waves<R, GUIDE>();
        constexpr int LDS = lds_bytes<R, WAVES, 2, F32Guide<GUIDE>::LUTW, kF32P, 16>();
        static_assert(WAVES >= 12, "tile does not fit LDS");
        return launch_c1_tiles<joint_f32_kernel<R, GUIDE, FMA>, LDS, WAVES, Geom<R, kF32P, 16>>(a, stream);
    });
}

int launch_joint_f32(int radius, int guide_channels, bool fma, const StencilArgs& a, hipStream_t s) {
    switch (guide_channels) {
        case 1:
            return fma ? launch_joint_f32_dispatch<1, true>(radius, a, s)
                       : launch_joint_f32_dispatch<1, false>(radius, a, s);
        case 3:
            return fma ? launch_joint_f32_dispatch<3, true>(radius, a, s)
                       : launch_joint_f32_dispatch<3, false>(radius, a, s);
        default: return VIP_ERR_INVALID_ARGUMENT;
    }
}

// ---------------------------------------------------------------- runtime radius
// 4 consecutive pixels of the two planes: guide words (colour distance) and floats (sums)
struct F32RtWin {
    uint32_t g[4];
    float c[4];
    __device__ __forceinline__ void load(const uint32_t* gplane, const uint32_t* fplane, int off) {
        const uint4 v = *reinterpret_cast<const uint4*>(gplane + off);
        const uint4 u = *reinterpret_cast<const uint4*>(fplane + off);
        g[0] = v.x; g[1] = v.y; g[2] = v.z; g[3] = v.w;
        c[0] = __uint_as_float(u.x); c[1] = __uint_as_float(u.y);
        c[2] = __uint_as_float(u.z); c[3] = __uint_as_float(u.w);
    }
};

// the joint filter's largest radius (ksize 47) is the runtime kernel's largest LDS footprint
constexpr int kF32RtMaxRadius = 23;
template <int GUIDE>
constexpr long long f32_rt_lds_bytes(int R) {
    const int L = round_up(R, 4);
    return 4LL * (2 * rt_plane_words(R, L, rt_stride(L)) + F32Guide<GUIDE>::LUTW);
}

template <int GUIDE, bool FMA>
__global__ __launch_bounds__(kRtWaves * 64) void joint_f32_rt_kernel(const RtArgs a) {
    using W = F32Guide<GUIDE>;
    static_assert(f32_rt_lds_bytes<GUIDE>(kF32RtMaxRadius) <= kLdsBudget, "planes and LUT do not fit LDS");
    constexpr int P = kRtP, NT = kRtWaves * 64, TH = kRtWaves * 4;
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const int R = a.R, L = a.L, S = a.S;
    const int rows = TH + 2 * R;
    const int pw = rt_plane_words(R, L, S);
    uint32_t* const gplane = lds;
    uint32_t* const fplane = lds + pw;
    uint32_t* const lut = lds + 2 * pw;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tx = lane & 15;
    const int ty = wave * 4 + (lane >> 4);
    const int tile = blockIdx.x;
    const int tx0 = (tile % a.tiles_x) * kRtTW, ty0 = (tile / a.tiles_x) * TH;

    // colour LUT: word d * COPIES + c = color[d]
    for (int q = tid; q < W::LUTW / 4; q += NT) {
        const uint32_t v = __float_as_uint(a.color[q >> (W::COPIES == 32 ? 3 : 2)]);
        *reinterpret_cast<uint4*>(lut + 4 * q) = make_uint4(v, v, v, v);
    }
    // tile planes; columns [TW + 2L, S) and the pad are zeroed: the last tap block of a row
    // reads up to 4 words past its apron (weight 0); a zero guide word's distance to any centre
    // stays inside the LUT (d <= 255, or 765 with a 3-channel guide) and a zero float times a
    // zero weight adds nothing
    {
        const int gpr = S / 4, valid = (kRtTW + 2 * L) / 4;
        const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
        for (int q = tid; q < rows * gpr; q += NT) {
            const int r = q / gpr, gc = q - r * gpr;
            uint4 gw = zero, fw = zero;
            if (gc < valid) {
                const int sy = clampi(ty0 + a.src_row0 - R + r, a.row_lo, a.row_hi - 1);
                F32Group<GUIDE> grp;
                grp.load(a.src, a.src_pitch, a.guide, a.guide_pitch, sy, tx0 - L + 4 * gc, a.width, a.aligned);
                gw = grp.words();
                fw = grp.source_words();
            }
            *reinterpret_cast<uint4*>(gplane + r * S + 4 * gc) = gw;
            *reinterpret_cast<uint4*>(fplane + r * S + 4 * gc) = fw;
        }
        if (L < 4 && tid < 2) {
            *reinterpret_cast<uint4*>(gplane + rows * S + 4 * tid) = zero;
            *reinterpret_cast<uint4*>(fplane + rows * S + 4 * tid) = zero;
        }
    }
    __syncthreads();
    if (ty0 + wave * 4 >= a.out_rows) return;  // wave-uniform; no barrier follows

    const int xc = L + tx * P;  // plane column of the thread's output 0
    uint32_t ctr[P];
    {
        const uint4 v = *reinterpret_cast<const uint4*>(gplane + (ty + R) * S + xc);
        ctr[0] = v.x; ctr[1] = v.y; ctr[2] = v.z; ctr[3] = v.w;
    }
    const uint32_t lanec = (uint32_t)(lane & (W::COPIES - 1)) << 2;
    const char* const lut_bytes = reinterpret_cast<const char*>(lut);

    float s[P], sk[P];
#pragma unroll
    for (int i = 0; i < P; ++i) s[i] = sk[i] = 0.f;

    // 4 taps x 4 outputs: tap t of the block pairs output i with pixel t + i of cur|nxt
    auto block = [&](const F32RtWin& cur, const F32RtWin& nxt, const kconst float* wsb) {
        const float wsv[4] = {wsb[0], wsb[1], wsb[2], wsb[3]};  // uniform: one scalar load
        float wc[4][P];
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int i = 0; i < P; ++i) {
                const int j = t + i;
                const uint32_t d = __builtin_amdgcn_sad_u8(j < 4 ? cur.g[j & 3] : nxt.g[j & 3], ctr[i], 0u);
                wc[t][i] = *reinterpret_cast<const float*>(lut_bytes + ((d << W::LUT_SHIFT) | lanec));
            }
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int i = 0; i < P; ++i) {
                const int j = t + i;
                const float n = j < 4 ? cur.c[j & 3] : nxt.c[j & 3];
                const float w = wc[t][i] * wsv[t];
                if constexpr (FMA)
                    s[i] = __builtin_fmaf(n, w, s[i]);
                else
                    s[i] = s[i] + n * w;
                sk[i] = sk[i] + w;
            }
    };

    for (int ky = -R; ky <= R; ++ky) {
        const int aky = ky < 0 ? -ky : ky;
        set_progress_priority((ky + R) * 4 / (2 * R + 1));
        const int hw = ((const kconst int*)a.hw)[aky];
        const int k4 = (hw + 3) & ~3;
        const int nblk = ((hw + k4) >> 2) + 1;  // blocks cover kx = -k4 .. -k4 + 4 nblk - 1 >= hw
        const kconst float* const wsr = (const kconst float*)a.wsrow + (ky + R) * a.wst + (a.ra - k4);
        const int off = (ty + R + ky) * S + xc - k4;
        F32RtWin A, B;
        A.load(gplane, fplane, off);
        int b = 0;
        for (; b + 2 <= nblk; b += 2) {  // two blocks per trip: the windows swap roles
            B.load(gplane, fplane, off + 4 * (b + 1));
            block(A, B, wsr + 4 * b);
            A.load(gplane, fplane, off + 4 * (b + 2));
            block(B, A, wsr + 4 * (b + 1));
        }
        if (b < nblk) {
            B.load(gplane, fplane, off + 4 * (b + 1));
            block(A, B, wsr + 4 * b);
        }
    }

    float o[P];
#pragma unroll
    for (int i = 0; i < P; ++i) o[i] = s[i] / sk[i];
    store_f32(a, ty0 + ty, tx0 + tx * P, o);
}

template <int GUIDE, bool FMA>
static int launch_joint_f32_rt_g(RtArgs a, hipStream_t stream) {
    if (a.R > kF32RtMaxRadius) return VIP_ERR_UNSUPPORTED_KSIZE;
    if (const int rc = rt_prepare(a)) return rc;
    const long long lds = 4LL * (2 * rt_plane_words(a.R, a.L, a.S) + F32Guide<GUIDE>::LUTW);
    return launch_rt_tiles<joint_f32_rt_kernel<GUIDE, FMA>>(a, lds, stream);
}

int launch_joint_f32_rt(const RtArgs& a, int guide_channels, bool fma, hipStream_t s) {
    switch (guide_channels) {
        case 1: return fma ? launch_joint_f32_rt_g<1, true>(a, s) : launch_joint_f32_rt_g<1, false>(a, s);
        case 3: return fma ? launch_joint_f32_rt_g<3, true>(a, s) : launch_joint_f32_rt_g<3, false>(a, s);
        default: return VIP_ERR_INVALID_ARGUMENT;
    }
}

}  // namespace vip
