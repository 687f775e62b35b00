// Confidence-weighted joint bilateral filter of an f32 one-channel source under an 8-bit guide,
// for gfx950 (MI355X): the normalised form of vip_joint_f32.hip's filter, which fills holes.
//
// Definition (include/vip.h, vip_joint_bilateral_run_conf_f32): per pixel, once,
// p = (c == 0) ? +0 : f * c; per output pixel and per tap in row-major order over the k x k
// square, w = ws[ky,kx] * wc[d], s = fmaf(p_n, w, s) and sumk = fmaf(c_n, w, sumk) (CUDA profile)
// or s + p_n * w and sumk + c_n * w (CPP profile); dst = (sumk == 0) ? hole_value : s / sumk
// (IEEE binary32 division), weight = sumk; replicate border, d as in vip_joint_f32.hip. Every
// weight and every LDS address comes from the guide, so neither f nor c can move an address. The
// build's -O3 -ffp-contract=off leaves the kernels in denorm mode 3: gradual underflow.
//
// Three LDS planes of one word per pixel: the guide word, p and c. The product and the c == 0
// select happen once per pixel, when the prefetch commits (ConfGroup::product_words); a tap then
// reads p and c as joint_f32_kernel reads f, one more ds_read_b128 per 4 neighbours, and sumk's
// add becomes an fma (CUDA profile: the same VALU count per tap as joint_f32_kernel).
//
// LDS budget (kLdsBudget = 160 KiB; planes of 4 bytes per pixel each). With three planes LDS
// alone allows (pick_waves, PLANES = 3)
//   gray guide, 256 x 32 LUT copies        16 waves to R = 4, 12 to R = 11, 8 to R = 15
//   3-channel guide, 768 x 16 LUT copies   16 waves to R = 2, 12 to R = 8, 8 to R = 13, 4 at R = 14, 15
//   3-channel guide, 768 x 8 LUT copies    16 waves to R = 7, 12 to R = 12, 8 to R = 15
// and the registers lower that where the staged prefetch (9 VGPRs per 4-pixel group with a gray
// guide, 11 with a 3-channel one) no longer fits beside the taps without scratch. What the kernels
// run (conf_waves, conf_rgb_copies; profiles/joint_conf_resources.txt):
//   gray guide       16 waves (128 x 64 tiles) to R = 3, 12 (128 x 48) to R = 9, 8 (128 x 32) to R = 15
//   3-channel guide  16 waves to R = 2, 12 to R = 8, 8 to R = 15; 16 LUT copies to R = 13, 8 at R = 14, 15
//
// Kernels:
//   joint_conf_f32_kernel<R, GUIDE, FMA>   radius 1..15; joint_f32_kernel's frame: persistent
//       workgroups over 128-pixel-wide tiles, 8 outputs per thread, the LUT in LDS, the next tile's
//       HBM reads in flight under the current tile's taps, xcd_tile's placement. Two stores per
//       output; a wave-uniform branch on the weight pointer guards the second.
//   joint_conf_f32_k1_kernel<FMA>          ksize 1: no neighbours, no guide read; elementwise.
// There is no runtime-radius kernel: ksize stops at 31 (kMaxKsizeJointConf).
//
// The tile prefetch, the tap loop of a tile row and the persistent launch are the one-channel
// kernels' own (vip_gray.hpp C1Prefetch and gray_row_taps, vip_launch.hpp launch_c1_tiles), which take
// a third plane as a policy of the GROUP and the DIST (THREE: ConfGroup and ConfSad below) and the
// kernel's argument struct as a template argument; for every two-plane type that text is
// discarded at compile time, and the assembly of the units that include vip_gray.hpp is the
// parent's (profiles/joint_conf_isa.txt). Guide4 / F32Group, RowStream, LutStage, Geom, pick_waves,
// xcd_tile, for_each_row and store_f32 are used as they are.
#include "vip_gray.hpp"

namespace vip {

constexpr int kConfP = 8;

// The colour LUT's form (as vip_joint_f32.hip's F32Guide, plus an 8-copy form): a gray guide
// reaches 256 entries and keeps 32 copies (conflict-free); a 3-channel guide reaches 768 and keeps
// 16 copies (lanes l and l + 16 share one: <= 2-way bank conflicts), or 8 (<= 4-way) at the radii
// where 16 copies leave LDS for 4 waves only (R = 14, 15: 8 copies fit 8 waves). Measured at 4K,
// 16 against 8 copies (profiles/joint_conf_4k_ab.txt): 86.8 / 105.1 us at ksize 9, 316.2 / 397.1 at
// 19 (the same waves, more bank conflicts), 1345.2 / 1048.5 at 31 (4 against 8 waves).
// (The two one-form builds were this function returning 16, or 8, at every radius.)
template <int R>
constexpr int conf_rgb_copies() {
    return R >= 14 ? 8 : 16;
}
template <int GUIDE, int R>
struct ConfGuide {
    static_assert(GUIDE == 1 || GUIDE == 3, "guide channels");
    static constexpr int ENTRIES = GUIDE == 3 ? 768 : 256;
    static constexpr int COPIES = GUIDE == 3 ? conf_rgb_copies<R>() : 32;
    static_assert(COPIES == 8 || COPIES == 16 || COPIES == 32, "copies");
    static constexpr int LUT_SHIFT = COPIES == 32 ? 7 : (COPIES == 16 ? 6 : 5);  // byte address: d << LUT_SHIFT | 4 * copy
    static constexpr int LUTW = ENTRIES * COPIES;
};

// Waves per workgroup: the most whose three planes fit LDS, and fewer from the radius on at which
// that workgroup's registers (16 waves: 128 VGPRs, 12: 168, 8: 256) no longer hold the kernel
// without scratch: with a gray guide 16 waves spill at R = 4 and 12 waves at R = 10, 11; with a
// 3-channel guide LDS binds first (profiles/joint_conf_resources.txt).
constexpr int kConfMax16Gray = 3, kConfMax16Rgb = 2;
constexpr int kConfMax12Gray = 9, kConfMax12Rgb = 8;
template <int R, int GUIDE>
constexpr int conf_waves() {
    constexpr int M16 = GUIDE == 3 ? kConfMax16Rgb : kConfMax16Gray;
    constexpr int M12 = GUIDE == 3 ? kConfMax12Rgb : kConfMax12Gray;
    return pick_waves<R, 3, (R <= M16 ? 16 : (R <= M12 ? 12 : 8)), ConfGuide<GUIDE, R>::LUTW, kConfP, 16>();
}

// 4 pixels of one image row: F32Group's guide dwords and source floats, and the confidence's 4
// floats, as loaded from HBM; words() is the guide plane's, source_words() the p plane's (the
// product, formed here once per pixel) and conf_words() the c plane's. C1Prefetch's GROUP.
template <int GUIDE>
struct ConfGroup {
    static constexpr bool TWO = true, THREE = true;  // guide, source (p) and confidence planes
    F32Group<GUIDE> fg;
    float4 c;

    __device__ __forceinline__ void load(const ConfArgs& a, int sy, int x) {
        fg.load(a.src, a.src_pitch, a.guide, a.guide_pitch, sy, x, a.width, a.aligned);
        const float* crow = reinterpret_cast<const float*>(a.conf + (long long)sy * a.conf_pitch);
        if (a.conf_vec && x >= 0 && x + 3 < a.width) {
            c = *reinterpret_cast<const float4*>(crow + x);
        } else {
            c.x = crow[clampi(x + 0, 0, a.width - 1)];
            c.y = crow[clampi(x + 1, 0, a.width - 1)];
            c.z = crow[clampi(x + 2, 0, a.width - 1)];
            c.w = crow[clampi(x + 3, 0, a.width - 1)];
        }
    }
    // p = (c == 0) ? +0 : f * c: one binary32 product; where c == 0 (-0 included) f is not a number
    __device__ __forceinline__ static uint32_t product(float f, float c) {
        return c == 0.f ? 0u : __float_as_uint(f * c);
    }
    __device__ __forceinline__ uint4 words() const { return fg.words(); }
    __device__ __forceinline__ uint4 source_words() const {
        return make_uint4(product(fg.f.x, c.x), product(fg.f.y, c.y), product(fg.f.z, c.z), product(fg.f.w, c.w));
    }
    __device__ __forceinline__ uint4 conf_words() const {
        return make_uint4(__float_as_uint(c.x), __float_as_uint(c.y), __float_as_uint(c.z), __float_as_uint(c.w));
    }
};

// A tap's colour-LUT index, gray_row_taps' DIST (as vip_joint_f32.hip's F32Sad, with the LUT form a
// template argument): the guide plane's word is the bare guide, the p plane's word the neighbour's
// product; THREE: the neighbour's confidence comes from a third plane and weighs sumk.
template <int LUT_SHIFT_, int P>
struct ConfSad {
    static constexpr bool TWO = true, THREE = true;
    static constexpr int LUT_SHIFT = LUT_SHIFT_;
    uint32_t ctr[P];  // the outputs' centre guide words
    __device__ __forceinline__ static uint32_t guide(uint32_t w) { return w; }
    __device__ __forceinline__ static float source(uint32_t w) { return __uint_as_float(w); }
    __device__ __forceinline__ uint32_t index(uint32_t g, float, int i) const {
        return __builtin_amdgcn_sad_u8(g, ctr[i], 0u);
    }
};

// What store_f32 reads of its argument struct: one float destination of the frame
struct ConfOut {
    uint8_t* dst;
    long long dst_pitch;
    int dst_aligned, out_rows, width;
};

template <int R, int GUIDE, bool FMA>
__global__ __launch_bounds__((conf_waves<R, GUIDE>() * 64)) void joint_conf_f32_kernel(const ConfArgs a) {
    using W = ConfGuide<GUIDE, R>;
    constexpr int P = kConfP, WAVES = conf_waves<R, GUIDE>(), NT = WAVES * 64;
    using G = Geom<R, P, 16>;
    constexpr int TH = WAVES * G::RPW;
    constexpr int ROWS = TH + 2 * R;
    static_assert(WAVES >= 4 && lds_bytes<R, WAVES, 3, W::LUTW, P, 16>() <= kLdsBudget, "three planes and the LUT fit LDS");
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    uint32_t* const lut = lds;
    uint32_t* const gplane = lds + W::LUTW;
    uint32_t* const pplane = gplane + ROWS * G::S;
    uint32_t* const cplane = pplane + ROWS * G::S;

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
    C1Prefetch<R, ROWS, NT, P, ConfGroup<GUIDE>> pf;
    std::conditional_t<W::COPIES == 8, LutStage8<NT, W::ENTRIES>,
                       LutStage<NT, W::ENTRIES, W::COPIES == 8 ? 16 : W::COPIES>> ls;
    ls.load(a.color);
    {
        const int t = xcd_tile(tile, a.tiles_total);
        pf.issue(a, (t % a.tiles_x) * G::TW, (t / a.tiles_x) * TH);
    }
    ls.store(lut);
    pf.commit(gplane, pplane, cplane);
    __syncthreads();

    for (;;) {
        const int t = xcd_tile(tile, a.tiles_total);
        const int tx0 = (t % a.tiles_x) * G::TW, ty0 = (t / a.tiles_x) * TH;
        const int next = tile + (int)gridDim.x;
        if (next < a.tiles_total) {  // next tile's HBM reads fly under this tile's taps
            const int n = xcd_tile(next, a.tiles_total);
            pf.issue(a, (n % a.tiles_x) * G::TW, (n / a.tiles_x) * TH);
        }
        if (ty0 + wave * G::RPW < a.out_rows) {  // wave-uniform: skip rows past the frame
            ConfSad<W::LUT_SHIFT, P> dist;
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
                // as joint_f32_kernel: every row of a plane is one base register plus a ds_read immediate
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
                gray_row_taps<HW, G::L, C0, NC, FMA, P>(gplane, pplane, row_off, wsv, lut_bytes, lanec, dist, s, sk,
                                                        cplane);
                // pin the accumulators at the row's end (fence_accumulators)
#pragma unroll
                for (int i = 0; i < P; ++i) __asm__ volatile("" : "+v"(s[i]), "+v"(sk[i]));
            });

            float o[P];
#pragma unroll
            for (int i = 0; i < P; ++i) o[i] = sk[i] == 0.f ? a.hole_value : s[i] / sk[i];
            store_f32(ConfOut{a.dst, a.dst_pitch, a.dst_aligned, a.out_rows, a.width}, ty0 + ty, tx0 + tx * P, o);
            if (a.weight)  // uniform over the grid
                store_f32(ConfOut{a.weight, a.weight_pitch, a.weight_aligned, a.out_rows, a.width}, ty0 + ty,
                          tx0 + tx * P, sk);
        }
        if (next >= a.tiles_total) break;
        __syncthreads();  // every wave is done reading this tile
        pf.commit(gplane, pplane, cplane);
        __syncthreads();
        tile = next;
    }
}

// ksize 1: the one tap has w = ws[0,0] * wc[0] = 1 (both LUTs hold exactly 1 there), so
// s = 0 + p and sumk = 0 + c (a -0 confidence gives sumk = +0); the guide is not read.
constexpr int kConfK1Threads = 256;
constexpr int kConfK1MaxGridY = 65535;  // rows beyond it stride over grid.y
template <bool FMA>
__global__ __launch_bounds__(kConfK1Threads) void joint_conf_f32_k1_kernel(const ConfArgs a) {
    const int x = (int)(blockIdx.x * kConfK1Threads + threadIdx.x);
    if (x >= a.width) return;
    const float w = a.ws[0] * a.color[0];
    for (int y = (int)blockIdx.y; y < a.out_rows; y += (int)gridDim.y) {
        const float f = reinterpret_cast<const float*>(a.src + (long long)y * a.src_pitch)[x];
        const float c = reinterpret_cast<const float*>(a.conf + (long long)y * a.conf_pitch)[x];
        const float p = __uint_as_float(ConfGroup<1>::product(f, c));
        float s, sk;
        if constexpr (FMA) {
            s = __builtin_fmaf(p, w, 0.f);
            sk = __builtin_fmaf(c, w, 0.f);
        } else {
            s = 0.f + p * w;
            sk = 0.f + c * w;
        }
        reinterpret_cast<float*>(a.dst + (long long)y * a.dst_pitch)[x] = sk == 0.f ? a.hole_value : s / sk;
        if (a.weight) reinterpret_cast<float*>(a.weight + (long long)y * a.weight_pitch)[x] = sk;
    }
}

template <bool FMA>
static int launch_conf_k1(const ConfArgs& a, hipStream_t stream) {
    note_launch(reinterpret_cast<const void*>(joint_conf_f32_k1_kernel<FMA>));
    if (a.width <= 0 || a.out_rows <= 0) return 0;
    const dim3 grid((unsigned)((a.width + kConfK1Threads - 1) / kConfK1Threads),
                    (unsigned)(a.out_rows < kConfK1MaxGridY ? a.out_rows : kConfK1MaxGridY));
    launch(joint_conf_f32_k1_kernel<FMA>, grid, dim3(kConfK1Threads), 0u, stream, a);
    return (int)hipGetLastError();
}

template <int GUIDE, bool FMA>
static int launch_joint_conf_dispatch(int radius, const ConfArgs& a, hipStream_t stream) {
    if (radius == 0) return launch_conf_k1<FMA>(a, stream);
    return dispatch_radius(radius, [&](auto rc) {
        constexpr int R = decltype(rc)::value, WAVES = conf_waves<R, GUIDE>();
        constexpr int LDS = lds_bytes<R, WAVES, 3, ConfGuide<GUIDE, R>::LUTW, kConfP, 16>();
        return launch_c1_tiles<joint_conf_f32_kernel<R, GUIDE, FMA>, LDS, WAVES, Geom<R, kConfP, 16>>(a, stream);
    });
}

int launch_joint_conf_f32(int radius, int guide_channels, bool fma, const ConfArgs& a, hipStream_t s) {
    switch (guide_channels) {
        case 1:
            return fma ? launch_joint_conf_dispatch<1, true>(radius, a, s)
                       : launch_joint_conf_dispatch<1, false>(radius, a, s);
        case 3:
            return fma ? launch_joint_conf_dispatch<3, true>(radius, a, s)
                       : launch_joint_conf_dispatch<3, false>(radius, a, s);
        default: return VIP_ERR_INVALID_ARGUMENT;
    }
}

}  // namespace vip
