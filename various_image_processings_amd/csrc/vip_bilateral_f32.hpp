// Self-guided bilateral filter of an f32 one-channel image, for gfx950 (MI355X): the float image
// is its own guide (a depth or disparity map on its own, an HDR luminance plane, a height field).
//
// Definition (include/vip.h, vip_bilateral_f32_run): N = VIP_BILATERAL_F32_BINS; per output pixel
// and per tap in row-major order over the k x k square, replicate border,
//   d = |f_n - f_c|;  t = min(d * scale, (float)N);  i = (int)t;  a = t - (float)i  (exact)
//   wc = fmaf(a, D[i], L[i]) (CUDA profile) or L[i] + a * D[i] (CPP profile)
//   w = ws[ky,kx] * wc;  s = fmaf(f_n, w, s) or s + f_n * w;  sumk += w;  dst = s / sumk
// with the range table L (the colour weight at difference i / scale) and its slopes
// D[i] = L[i + 1] - L[i], built on the host. The build's -O3 -ffp-contract=off leaves the kernels in
// denorm mode 3 (.amdhsa_float_denorm_mode_32 3): gradual underflow, as the definition.
//
// This is the one kernel of the f32 family whose LDS table address comes from the source value, not
// from an 8-bit guide. The index is bounded for every bit pattern of the source by the tap's
// v_min_f32: u = d * scale is the result of a multiply, so it is a number >= +0, +Inf or a quiet
// NaN, and v_min_f32(u, 1024.0) returns the other operand when one is a NaN: t lies in [0, N]
// whatever f holds, v_cvt_i32_f32 of it in 0..N, and the table has N + 1 pairs. (The conversion
// saturates and maps a NaN to 0 on its own account.)
//
// One LDS plane of one float per pixel (the gray kernels' Geom, row strides and ds_read_b128 row
// stream carry over), and the range table as (L[i], D[i]) pairs, so that one ds_read_b64 gives
// both: pair i, copy c at byte (i << 6) | (c << 3), c = lane & 7.
//   Copies: the ds_read_b64 bank rule is 32-lane groups, bank (address / 4) mod 64, two banks per
//   lane. A pair entry of 8 copies spans 16 banks, so the 4 lanes of a 32-lane group that share a
//   copy meet in one bank pair only when their indices are equal mod 4 and differ (equal indices
//   are one address). 16 copies (131,200 B) would leave LDS for no 16-wave plane at any radius
//   (R = 1: 36,960 B of plane, 168,160 B in all), 32 copies fit no CU. So 8 copies at every radius.
//
// LDS budget (kLdsBudget = 160 KiB): the table is 1025 x 8 x 8 = 65,600 B; the plane at R = 15 with
// 16 waves is (64 + 30) x 164 x 4 = 61,664 B: 127,264 B, so LDS allows 16 waves at every radius;
// the wave count is what the registers allow (bf32_waves; profiles/bilateral_f32_resources.txt).
//
// bilateral_f32_kernel<R, FMA>, R = 1..15: joint_f32_kernel's frame with one plane: persistent
// workgroups over 128-wide tiles, 8 outputs per thread, every tile row straight-line code (Geom,
// for_each_row, RowStream), the next tile's HBM reads in flight under the current tile's taps
// (C1Prefetch), xcd_tile's placement. R = 0 (ksize 1) is elementwise: the one tap has t = 0, a = 0,
// wc = L[0], so no table read and no LDS. There is no runtime-radius kernel: ksize stops at 31.
// The tap loop is this kernel's own (bf32_row_taps): gray_row_taps reads one LUT word per tap at an
// integer distance, this one a pair at a float one, and the interpolation stands between the read
// and the weight.
#pragma once

#include "vip_gray.hpp"

namespace vip {

constexpr int kBf32P = 8;
constexpr int kBf32Bins = VIP_BILATERAL_F32_BINS;
constexpr int kBf32Copies = 8;                          // interleaved copies of each pair
constexpr int kBf32Shift = 6;                           // pair byte address: i << 6 | 8 * copy
constexpr int kBf32LutW = kBf32Pairs * 2 * kBf32Copies; // LDS words of the table
static_assert(kBf32Copies * 8 == 1 << kBf32Shift, "pair address: i << 6");
static_assert(kBf32Pairs == kBf32Bins + 1, "pairs i = 0..N");

// Waves per workgroup: 16 while a 16-wave workgroup's 128 VGPRs hold the kernel without scratch,
// 12 (168 VGPRs, 128 x 48 tiles) above (profiles/bilateral_f32_resources.txt)
constexpr int kBf32Max16 = 15;
template <int R>
constexpr int bf32_waves() {
    return pick_waves<R, 1, (R <= kBf32Max16 ? 16 : 12), kBf32LutW, kBf32P, 16>();
}

// 4 pixels of one image row from column x (columns clamped to the image) as loaded from HBM, which
// are the plane words as they stand (F32Group's float loads without a guide). C1Prefetch's GROUP.
struct Bf32Group {
    static constexpr bool TWO = false;  // one plane
    float4 f;

    __device__ __forceinline__ void load(const uint8_t* src, long long src_pitch, const uint8_t*, long long, int sy,
                                         int x, int width, int aligned) {
        const float* frow = reinterpret_cast<const float*>(src + (long long)sy * src_pitch);
        if ((aligned & kF32SrcVec) && x >= 0 && x + 3 < width) {
            f = *reinterpret_cast<const float4*>(frow + x);
        } else {
            f.x = frow[clampi(x + 0, 0, width - 1)];
            f.y = frow[clampi(x + 1, 0, width - 1)];
            f.z = frow[clampi(x + 2, 0, width - 1)];
            f.w = frow[clampi(x + 3, 0, width - 1)];
        }
    }
    __device__ __forceinline__ uint4 words() const {
        return make_uint4(__float_as_uint(f.x), __float_as_uint(f.y), __float_as_uint(f.z), __float_as_uint(f.w));
    }
};

// LutStage for the pair table: words i * 16 + 2 c, + 1 = (L[i], D[i]); a uint4 store writes two
// copies, four stores a pair. load() issues a thread's table reads at once, store() writes them.
template <int NT>
struct PairStage {
    static constexpr int N = kBf32Pairs * kBf32Copies / 2;  // uint4 stores
    static constexpr int K = (N + NT - 1) / NT;
    uint2 v[K];
    __device__ __forceinline__ void load(const float* pairs) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int q = (int)threadIdx.x + k * NT;
            if (N % NT == 0 || q < N) v[k] = reinterpret_cast<const uint2*>(pairs)[q >> 2];
        }
    }
    __device__ __forceinline__ void store(uint32_t* lut) const {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int q = (int)threadIdx.x + k * NT;
            if (N % NT == 0 || q < N) *reinterpret_cast<uint4*>(lut + 4 * q) = make_uint4(v[k].x, v[k].y, v[k].x, v[k].y);
        }
    }
};

// The tap loop of one tile row (gray_row_taps' frame: neighbour column j serves output i at
// kx = j - L - i, per output the taps run in ascending kx, the pair reads kPipeDepth columns ahead
// of their use). cf: the outputs' centre values; lane8: 8 * the lane's table copy.
template <int HW, int L, int C0, int NC, bool FMA, int P>
__device__ __forceinline__ void bf32_row_taps(const uint32_t* plane, int row_off, const float (&wsv)[HW + 1],
                                              const char* lut, uint32_t lane8, float scale, const float (&cf)[P],
                                              float (&s)[P], float (&sk)[P]) {
    constexpr int D = kPipeDepth, NB = D + 1;
    constexpr int J0 = L - HW, J1 = L + P - 1 + HW;
    constexpr int LA = D + kRowLookahead;
    static_assert(J0 >= 4 * C0 && J1 < 4 * (C0 + NC), "row chunk range");
    auto chunk = [](int j) constexpr { return (j - 4 * C0) >> 2; };
    constexpr int PRE = chunk(J0 + LA < J1 ? J0 + LA : J1);
    RowStream<C0, NC, false> row(plane, plane, row_off);
#pragma unroll
    for (int q = 0; q <= PRE; ++q) row.load(q);
    float2 pr[NB][P];
    float av[NB][P], nf[NB];
    auto issue = [&](int j) {
        const int b = (j - J0) % NB;
        nf[b] = __uint_as_float(row.guide(j - 4 * C0));
#pragma unroll
        for (int i = 0; i < P; ++i) {
            const int kx = j - L - i;
            if (kx < -HW || kx > HW) continue;
            const float d = __builtin_fabsf(nf[b] - cf[i]);
            // v_min_f32: t in [0, N] for every bit pattern of the source (see the head of the file)
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

constexpr int kBf32K1Threads = 256;
constexpr int kBf32K1MaxGridY = 65535;  // rows beyond it stride over grid.y

template <int R>
constexpr int bf32_threads() {
    if constexpr (R == 0)
        return kBf32K1Threads;
    else
        return bf32_waves<R>() * 64;
}

template <int R, bool FMA>
__global__ __launch_bounds__((bf32_threads<R>())) void bilateral_f32_kernel(const BilateralF32Args a) {
    if constexpr (R == 0) {
        // ksize 1: the one tap has d = 0, t = 0, a = 0 and wc = fmaf(0, D[0], L[0]) = L[0] + 0 * D[0] = L[0]
        // (D[0] is finite), so w = ws[0,0] * L[0] = 1; no address is formed from the source
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
        constexpr int P = kBf32P, WAVES = bf32_waves<R>(), NT = WAVES * 64;
        using G = Geom<R, P, 16>;
        constexpr int TH = WAVES * G::RPW;
        constexpr int ROWS = TH + 2 * R;
        static_assert(WAVES >= 12 && lds_bytes<R, WAVES, 1, kBf32LutW, P, 16>() <= kLdsBudget,
                      "the plane and the pair table fit LDS");
        extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
        uint32_t* const lut = lds;
        uint32_t* const plane = lds + kBf32LutW;
        static_assert(kBf32LutW % 4 == 0, "the plane starts 16-byte aligned");

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
        C1Prefetch<R, ROWS, NT, P, Bf32Group> pf;
        PairStage<NT> ls;
        ls.load(a.color);
        {
            const int t = xcd_tile(tile, a.tiles_total);
            pf.issue(a, (t % a.tiles_x) * G::TW, (t / a.tiles_x) * TH);
        }
        ls.store(lut);
        pf.commit(plane);
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
                float cf[P];
                {
                    const uint4* c = reinterpret_cast<const uint4*>(plane + (ty + R) * G::S + tx * P + G::L);
#pragma unroll
                    for (int q = 0; q < P / 4; ++q) {
                        const uint4 v = c[q];
                        cf[4 * q + 0] = __uint_as_float(v.x);
                        cf[4 * q + 1] = __uint_as_float(v.y);
                        cf[4 * q + 2] = __uint_as_float(v.z);
                        cf[4 * q + 3] = __uint_as_float(v.w);
                    }
                }
                float s[P], sk[P];
#pragma unroll
                for (int i = 0; i < P; ++i) s[i] = sk[i] = 0.f;

                for_each_row<R, true>([&](const int ky, auto hwc) {
                    // as joint_f32_kernel: every row of the plane is one base register plus a ds_read immediate
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
                    bf32_row_taps<HW, G::L, C0, NC, FMA, P>(plane, row_off, wsv, lut_bytes, lane8, scale, cf, s, sk);
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
            pf.commit(plane);
            __syncthreads();
            tile = next;
        }
    }
}

template <bool FMA>
static int launch_bf32_k1(const BilateralF32Args& a, hipStream_t stream) {
    note_launch(reinterpret_cast<const void*>(bilateral_f32_kernel<0, FMA>));
    if (a.width <= 0 || a.out_rows <= 0) return 0;
    const dim3 grid((unsigned)((a.width + kBf32K1Threads - 1) / kBf32K1Threads),
                    (unsigned)(a.out_rows < kBf32K1MaxGridY ? a.out_rows : kBf32K1MaxGridY));
    launch(bilateral_f32_kernel<0, FMA>, grid, dim3(kBf32K1Threads), 0u, stream, a);
    return (int)hipGetLastError();
}

// The kernels are instantiated by eight small units, vip_bilateral_f32_fma_p0.hip .. _mul_p3.hip, one per
// arithmetic and radius group (kBf32PartLo / kBf32PartHi, vip_launch.hpp). A radius' kernel is one
// straight-line block per tile whose compile time grows with the square of its tap count (R = 15
// alone is a quarter of all 32 kernels' time), so the units split the work evenly and build in
// parallel; each defines its specialization of launch_bilateral_f32_part from launch_bf32_part below,
// and launch_bilateral_f32 (vip_launch.hpp) picks among them.
template <bool FMA, int PART>
static int launch_bf32_part(int radius, const BilateralF32Args& a, hipStream_t stream) {
    static_assert(PART >= 0 && PART < kBf32Parts, "radius group");
    constexpr int LO = kBf32PartLo[PART], HI = kBf32PartHi[PART];
    int rc = VIP_ERR_UNSUPPORTED_KSIZE;
    auto one = [&](auto rcst) {
        constexpr int R = decltype(rcst)::value;
        if constexpr (R == 0) {
            return launch_bf32_k1<FMA>(a, stream);
        } else {
            constexpr int WAVES = bf32_waves<R>();
            constexpr int LDS = lds_bytes<R, WAVES, 1, kBf32LutW, kBf32P, 16>();
            return launch_c1_tiles<bilateral_f32_kernel<R, FMA>, LDS, WAVES, Geom<R, kBf32P, 16>>(a, stream);
        }
    };
    [&]<int... I>(std::integer_sequence<int, I...>) {
        (void)(... || (radius == LO + I && (rc = one(std::integral_constant<int, LO + I>{}), true)));
    }(std::make_integer_sequence<int, HI - LO + 1>{});
    return rc;
}

}  // namespace vip
