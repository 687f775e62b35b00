// Joint bilateral filter of an f32 one-channel source under an f32 one-channel guide, for gfx950
// (MI355X): a noisy depth map under an HDR luminance plane, a flow component under a depth map, a
// radiance plane under its depth buffer. The handle is vip_bilateral_f32_t as it stands.
//
// Definition (include/vip.h, vip_bilateral_f32_run_joint): N = VIP_BILATERAL_F32_BINS; per output
// pixel and per tap in row-major order over the k x k square, replicate border on both images,
//   d = |g_n - g_c|;  t = min(d * scale, (float)N);  i = (int)t;  a = t - (float)i  (exact)
//   wc = fmaf(a, D[i], L[i]) (CUDA profile) or L[i] + a * D[i] (CPP profile)
//   w = ws[ky,kx] * wc;  s = fmaf(f_n, w, s) or s + f_n * w;  sumk += w;  dst = s / sumk
// with vip_bilateral_f32_create's tables. It is vip_bilateral_f32_run's definition with the
// distance taken from the guide g and the accumulated value from the source f; g == f gives that
// filter bit for bit.
//
// The LDS table address comes from the guide value, as the self-guided kernel's comes from its
// source. The index is bounded for every bit pattern of the guide by the tap's v_min_f32, by that
// kernel's argument: u = d * scale is the result of a multiply, so it is a number >= +0, +Inf or a
// quiet NaN, and v_min_f32(u, 1024.0) returns the other operand when one is a NaN: t lies in [0, N]
// whatever g holds, v_cvt_i32_f32 of it in 0..N, and the table has N + 1 pairs. No address is
// formed from the source f: it enters the accumulating fma only.
//
// Two LDS planes of one float per pixel, the guide's and then the source's (joint_f32_kernel's
// layout with a float guide plane: C1Prefetch on a GROUP with TWO, RowStream<..., true>), and the
// range table as (L[i], D[i]) pairs at byte (i << 6) | (c << 3), c = lane & 7, staged by PairStage:
// one ds_read_b64 per tap. The copies stay 8 at every radius (vip_bilateral_f32.hpp's bank
// argument; 16 copies leave no room for two planes).
//
// LDS budget (kLdsBudget = 163,840 B): the table is 65,600 B, which leaves 98,240 B or 12,280
// words per plane. Geom<R, 8, 16>: S = round_up(128 + 2 L, 8) + 4, L = round_up(R, 4):
//   R = 8:  S = 148, 16 waves (64 + 16) x 148 = 11,840 words            -> 16 waves up to R = 8
//   R = 9:  S = 156, 16 waves 82 x 156 = 12,792 (no), 12 waves 66 x 156 -> 12 waves for R = 9..13
//   R = 13: S = 164, 12 waves 74 x 164 = 12,136
//   R = 14: S = 164, 12 waves 76 x 164 = 12,464 (no), 8 waves 60 x 164  -> 8 waves for R = 14, 15
// pick_waves gives these counts, and the registers ask for fewer (kBf32jMaxWaves): beside the
// self-guided kernel's registers a thread holds the second row stream and twice the prefetch
// staging, and with the LDS counts R = 3..8 (128 VGPRs) and R = 9..13 (168 VGPRs) spill 44 to 164
// bytes of scratch. So 16 waves for R = 1, 2, 12 for R = 3..8 and 8 for R = 9..15: at most 120, 165
// and 222 VGPRs, 0 bytes of scratch in all 32 kernels (profiles/bilateral_f32j_resources.txt).
//
// bilateral_f32_joint_kernel<R, FMA>, R = 1..15: bilateral_f32_kernel's frame: persistent
// workgroups over 128-wide tiles, 8 outputs per thread, every tile row straight-line code, the next
// tile's HBM reads of both images staged in registers under the current tile's taps, xcd_tile's
// placement, store_f32. The 8 guide centre values stay in registers across the tile. A tap is the
// self-guided kernel's 11 VALU operations and its ds_read_b64; the only extra per neighbour column
// is the source plane's row stream. R = 0 (ksize 1) is elementwise: w = ws[0] * L[0],
// dst = fmaf(f, w, 0) / (0 + w); no table read, no LDS, and the guide is not read.
// The tap loop is this kernel's own (bf32j_row_taps), so that bf32_row_taps and the kernels built
// from it stay as they are.
#pragma once

#include "vip_bilateral_f32.hpp"

namespace vip {

// Waves per workgroup that the registers allow without scratch, by radius (pick_waves then checks
// LDS): a 16-wave workgroup has 128 VGPRs per thread, a 12-wave one 168, an 8-wave one 256
constexpr int kBf32jMaxWaves[kMaxRadius + 1] = {16, 16, 16, 12, 12, 12, 12, 12, 12, 8, 8, 8, 8, 8, 8, 8};
template <int R>
constexpr int bf32j_waves() {
    return pick_waves<R, 2, kBf32jMaxWaves[R], kBf32LutW, kBf32P, 16>();
}

// 4 pixels of one image row from column x (columns clamped to the image) of the guide and of the
// source as loaded from HBM, which are the two planes' words as they stand. C1Prefetch's GROUP.
// 16-byte loads where the image allows them, decided for each image on its own.
struct Bf32jGroup {
    static constexpr bool TWO = true;
    float4 g, f;

    __device__ __forceinline__ static float4 load4(const uint8_t* img, long long pitch, int sy, int x, int width,
                                                   bool vec) {
        const float* row = reinterpret_cast<const float*>(img + (long long)sy * pitch);
        if (vec && x >= 0 && x + 3 < width) return *reinterpret_cast<const float4*>(row + x);
        float4 v;
        v.x = row[clampi(x + 0, 0, width - 1)];
        v.y = row[clampi(x + 1, 0, width - 1)];
        v.z = row[clampi(x + 2, 0, width - 1)];
        v.w = row[clampi(x + 3, 0, width - 1)];
        return v;
    }
    __device__ __forceinline__ void load(const uint8_t* src, long long src_pitch, const uint8_t* guide,
                                         long long guide_pitch, int sy, int x, int width, int aligned) {
        g = load4(guide, guide_pitch, sy, x, width, (aligned & kF32GuideVec) != 0);
        f = load4(src, src_pitch, sy, x, width, (aligned & kF32SrcVec) != 0);
    }
    __device__ __forceinline__ uint4 words() const {
        return make_uint4(__float_as_uint(g.x), __float_as_uint(g.y), __float_as_uint(g.z), __float_as_uint(g.w));
    }
    __device__ __forceinline__ uint4 source_words() const {
        return make_uint4(__float_as_uint(f.x), __float_as_uint(f.y), __float_as_uint(f.z), __float_as_uint(f.w));
    }
};

// The tap loop of one tile row (bf32_row_taps' frame with two planes: the distance from the guide
// column, the accumulated value from the source column). cg: the outputs' centre guide values;
// lane8: 8 * the lane's table copy.
template <int HW, int L, int C0, int NC, bool FMA, int P>
__device__ __forceinline__ void bf32j_row_taps(const uint32_t* gplane, const uint32_t* fplane, int row_off,
                                               const float (&wsv)[HW + 1], const char* lut, uint32_t lane8,
                                               float scale, const float (&cg)[P], float (&s)[P], float (&sk)[P]) {
    constexpr int D = kPipeDepth, NB = D + 1;
    constexpr int J0 = L - HW, J1 = L + P - 1 + HW;
    constexpr int LA = D + kRowLookahead;
    static_assert(J0 >= 4 * C0 && J1 < 4 * (C0 + NC), "row chunk range");
    auto chunk = [](int j) constexpr { return (j - 4 * C0) >> 2; };
    constexpr int PRE = chunk(J0 + LA < J1 ? J0 + LA : J1);
    RowStream<C0, NC, true> row(gplane, fplane, row_off);
#pragma unroll
    for (int q = 0; q <= PRE; ++q) row.load(q);
    float2 pr[NB][P];
    float av[NB][P], nf[NB];
    auto issue = [&](int j) {
        const int b = (j - J0) % NB;
        const float ng = __uint_as_float(row.guide(j - 4 * C0));
        nf[b] = __uint_as_float(row.source(j - 4 * C0));
#pragma unroll
        for (int i = 0; i < P; ++i) {
            const int kx = j - L - i;
            if (kx < -HW || kx > HW) continue;
            const float d = __builtin_fabsf(ng - cg[i]);
            // v_min_f32: t in [0, N] for every bit pattern of the guide (see the head of the file)
            const float t = __builtin_fminf(d * scale, (float)kBf32Bins);
            const int e = (int)t;
            av[b][i] = t - (float)e;
            pr[b][i] = *reinterpret_cast<const float2*>(lut + (((uint32_t)e << kBf32Shift) | lane8));
        }
    };
#pragma unroll
    for (int j = J0; j < J0 + D && j <= J1; ++j) issue(j);
#pragma unroll
    for (int j = J0; j <= J1; ++j) {
        if (j + LA <= J1 && ((j + LA) & 3) == 0 && chunk(j + LA) > PRE) row.load(chunk(j + LA));
        if (j + D <= J1) issue(j + D);
        const int b = (j - J0) % NB;
#pragma unroll
        for (int i = 0; i < P; ++i) {
            const int kx = j - L - i;
            if (kx < -HW || kx > HW) continue;
            float wc;
            if constexpr (FMA)
                wc = __builtin_fmaf(av[b][i], pr[b][i].y, pr[b][i].x);
            else
                wc = pr[b][i].x + av[b][i] * pr[b][i].y;
            const float w = wsv[kx < 0 ? -kx : kx] * wc;
            if constexpr (FMA)
                s[i] = __builtin_fmaf(nf[b], w, s[i]);
            else
                s[i] = s[i] + nf[b] * w;
            sk[i] = sk[i] + w;
        }
        __builtin_amdgcn_sched_barrier(0);
    }
}

template <int R>
constexpr int bf32j_threads() {
    if constexpr (R == 0)
        return kBf32K1Threads;
    else
        return bf32j_waves<R>() * 64;
}

template <int R, bool FMA>
__global__ __launch_bounds__((bf32j_threads<R>())) void bilateral_f32_joint_kernel(const BilateralF32Args a) {
    if constexpr (R == 0) {
        // ksize 1: the one tap has d = |g_c - g_c|, which is 0 for a finite guide, so t = 0, a = 0 and
        // wc = L[0] in both profiles, w = ws[0,0] * L[0] = 1: the guide is not read, and no address is
        // formed from either image
        const int x = (int)(blockIdx.x * kBf32K1Threads + threadIdx.x);
        if (x >= a.width) return;
        const float w = a.ws[0] * a.color[0];
        for (int y = (int)blockIdx.y; y < a.out_rows; y += (int)gridDim.y) {
            const int sy = clampi(y + a.src_row0, a.row_lo, a.row_hi - 1);
            const float f = reinterpret_cast<const float*>(a.src + (long long)sy * a.src_pitch)[x];
            float s;
            if constexpr (FMA)
                s = __builtin_fmaf(f, w, 0.f);
            else
                s = 0.f + f * w;
            reinterpret_cast<float*>(a.dst + (long long)y * a.dst_pitch)[x] = s / (0.f + w);
        }
    } else {
        constexpr int P = kBf32P, WAVES = bf32j_waves<R>(), NT = WAVES * 64;
        using G = Geom<R, P, 16>;
        constexpr int TH = WAVES * G::RPW;
        constexpr int ROWS = TH + 2 * R;
        static_assert(WAVES >= 8 && lds_bytes<R, WAVES, 2, kBf32LutW, P, 16>() <= kLdsBudget,
                      "the two planes and the pair table fit LDS");
        extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
        uint32_t* const lut = lds;
        uint32_t* const gplane = lds + kBf32LutW;
        uint32_t* const fplane = gplane + ROWS * G::S;
        static_assert(kBf32LutW % 4 == 0 && (ROWS * G::S) % 4 == 0, "the planes start 16-byte aligned");

        const int tid = threadIdx.x;
        const int lane = tid & 63;
        const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
        const int tx = lane & 15;
        const int ty = wave * G::RPW + (lane >> 4);
        static_assert(G::S % 4 == 0 && P % 4 == 0, "plane rows in uint4");
        const int base4 = ty * (G::S / 4) + tx * (P / 4);  // uint4 index of the thread's tile row, column tx * P
        const uint32_t lane8 = (uint32_t)(lane & (kBf32Copies - 1)) << 3;  // this lane's table copy
        const char* const lut_bytes = reinterpret_cast<const char*>(lut);
        const float scale = a.scale;

        // persistent: workgroup b filters tiles b, b + grid, ... (xcd_tile's placement)
        int tile = blockIdx.x;
        C1Prefetch<R, ROWS, NT, P, Bf32jGroup> pf;
        PairStage<NT> ls;
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
            if (next < a.tiles_total) {  // next tile's HBM reads of both images fly under this tile's taps
                const int n = xcd_tile(next, a.tiles_total);
                pf.issue(a, (n % a.tiles_x) * G::TW, (n / a.tiles_x) * TH);
            }
            if (ty0 + wave * G::RPW < a.out_rows) {  // wave-uniform: skip rows past the band
                float cg[P];  // the outputs' centre guide values, in registers across the tile
                {
                    const uint4* c = reinterpret_cast<const uint4*>(gplane + (ty + R) * G::S + tx * P + G::L);
#pragma unroll
                    for (int q = 0; q < P / 4; ++q) {
                        const uint4 v = c[q];
                        cg[4 * q + 0] = __uint_as_float(v.x);
                        cg[4 * q + 1] = __uint_as_float(v.y);
                        cg[4 * q + 2] = __uint_as_float(v.z);
                        cg[4 * q + 3] = __uint_as_float(v.w);
                    }
                }
                float s[P], sk[P];
#pragma unroll
                for (int i = 0; i < P; ++i) s[i] = sk[i] = 0.f;

                for_each_row<R, true>([&](const int ky, auto hwc) {
                    // every row of either plane is one base register plus a ds_read immediate
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
                    bf32j_row_taps<HW, G::L, C0, NC, FMA, P>(gplane, fplane, row_off, wsv, lut_bytes, lane8, scale, cg,
                                                             s, sk);
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
}

template <bool FMA>
static int launch_bf32j_k1(const BilateralF32Args& a, hipStream_t stream) {
    note_launch(reinterpret_cast<const void*>(bilateral_f32_joint_kernel<0, FMA>));
    if (a.width <= 0 || a.out_rows <= 0) return 0;
    const dim3 grid((unsigned)((a.width + kBf32K1Threads - 1) / kBf32K1Threads),
                    (unsigned)(a.out_rows < kBf32K1MaxGridY ? a.out_rows : kBf32K1MaxGridY));
    launch(bilateral_f32_joint_kernel<0, FMA>, grid, dim3(kBf32K1Threads), 0u, stream, a);
    return (int)hipGetLastError();
}

// The kernels are instantiated by eight small units, vip_bilateral_f32j_fma_p0.hip .. _mul_p3.hip,
// one per arithmetic and radius group (kBf32jPartLo / kBf32jPartHi, vip_launch.hpp), for the reason
// vip_bilateral_f32.hpp gives: a radius' compile time grows with the square of its tap count. Each
// unit defines its specialization of launch_bilateral_f32_joint_part from launch_bf32j_part below,
// and launch_bilateral_f32_joint (vip_launch.hpp) picks among them.
template <bool FMA, int PART>
static int launch_bf32j_part(int radius, const BilateralF32Args& a, hipStream_t stream) {
    static_assert(PART >= 0 && PART < kBf32jParts, "radius group");
    constexpr int LO = kBf32jPartLo[PART], HI = kBf32jPartHi[PART];
    int rc = VIP_ERR_UNSUPPORTED_KSIZE;
    auto one = [&](auto rcst) {
        constexpr int R = decltype(rcst)::value;
        if constexpr (R == 0) {
            return launch_bf32j_k1<FMA>(a, stream);
        } else {
            constexpr int WAVES = bf32j_waves<R>();
            constexpr int LDS = lds_bytes<R, WAVES, 2, kBf32LutW, kBf32P, 16>();
            static_assert(LDS <= kLdsBudget, "the two planes and the pair table fit LDS");
            return launch_c1_tiles<bilateral_f32_joint_kernel<R, FMA>, LDS, WAVES, Geom<R, kBf32P, 16>>(a, stream);
        }
    };
    [&]<int... I>(std::integer_sequence<int, I...>) {
        (void)(... || (radius == LO + I && (rc = one(std::integral_constant<int, LO + I>{}), true)));
    }(std::make_integer_sequence<int, HI - LO + 1>{});
    return rc;
}

}  // namespace vip
