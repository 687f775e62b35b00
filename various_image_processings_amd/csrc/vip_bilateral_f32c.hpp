// Self-guided bilateral filter of an interleaved f32 image of C = 2 or 3 channels, for gfx950
// (MI355X): a float colour image is its own guide (linear-light or HDR RGB, a Lab frame, a normal
// map, a 2-channel flow field). vip_bilateral_f32.hpp's filter with the range weight of the colour
// kernels: one weight per tap, from the L1 distance over the channels.
//
// Definition (include/vip.h, vip_bilateral_f32_run_c): N = VIP_BILATERAL_F32_BINS; per output pixel
// and per tap in row-major order over the k x k square, replicate border,
//   d = |f_0(n) - f_0(c)| + |f_1(n) - f_1(c)|  (C = 3: ... + |f_2(n) - f_2(c)|, added left to right)
//   t = min(d * scale, (float)N);  i = (int)t;  a = t - (float)i  (exact)
//   wc = fmaf(a, D[i], L[i]) (CUDA profile) or L[i] + a * D[i] (CPP profile)
//   w = ws[ky,kx] * wc, formed once per tap;  s_c = fmaf(f_c(n), w, s_c) or s_c + f_c(n) * w for each
//   channel;  sumk += w once;  dst_c = s_c / sumk
// with the handle's tables exactly as the one-channel kernel reads them. The build's -O3
// -ffp-contract=off leaves the kernels in denorm mode 3 (gradual underflow) and fuses nothing: every
// subtract, abs, add and multiply above is a binary32 operation of its own.
//
// The LDS table address comes from the source values. The index is bounded for every bit pattern
// of the source by the tap's v_min_f32: d is a sum of absolute values, so it is a number >= +0,
// +Inf (also where a finite sum overflows) or a NaN; u = d * scale is the result of a multiply by a
// finite scale > 0, so it is again a number >= +0, +Inf or a quiet NaN, and v_min_f32(u, 1024.0)
// returns the other operand when one is a NaN: t lies in [0, N] whatever f holds, v_cvt_i32_f32 of
// it in 0..N, and the table has N + 1 pairs. (The conversion saturates and maps a NaN to 0 on its
// own account.)
//
// LDS: the pair table in the one-channel layout ((L[i], D[i]), pair i, copy c at byte
// (i << 6) | (c << 3), c = lane & 7, one ds_read_b64 per tap; PairStage fills it), then C one-word
// planes f_0 .. f_{C-1} with the one-channel kernels' row strides (Geom::S) and ds_read_b128 row
// stream. The source is de-interleaved once per pixel, when the prefetch commits
// (Bf32cGroup::channel_words), and re-interleaved at the store (store_bf32c): a thread's 8 outputs
// are 8 * C consecutive floats, 2 * C whole 16-byte groups where dst allows them.
//
// Wave count and table copies (kLdsBudget = 160 KiB): the table is 1025 x 8 x 8 = 65,600 B at 8
// copies, which leaves 98,240 B for the planes. The rule is vip_joint_f32c.hip's (F32cForm): the
// full copies are kept while at least 8 waves fit beside them, and only else halved. Here 8 waves
// fit at every (C, R): the largest planes, C = 3 at R = 5..7, are 3 x 46 x 148 x 4 = 81,696 B with
// 8 waves (12 waves: 110,112 B, too many), C = 3 at R <= 4 holds 12 waves (R = 4: 94,080 B) and
// C = 2 up to 16 (R = 7: 92,352 B). So the copies are never halved (a static_assert in Bf32cForm)
// and the ds_read_b64 bank argument is the one-channel header's for 8 copies, unchanged: 32-lane
// groups, two banks per lane, the 4 lanes that share a copy meet in one bank pair only when their
// indices are equal mod 4 and differ. The wave count is then the largest that LDS allows
// (pick_waves) and the registers hold without scratch (bf32c_max_waves): against the one-channel
// kernel a thread holds 8 * (C - 1) more accumulators, as many more centre values and C times the
// staged prefetch. profiles/bilateral_f32c_resources.txt has every kernel's registers, LDS and
// scratch (0).
//
// Kernels:
//   bilateral_f32c_kernel<R, C, FMA>   radius 1..7: bilateral_f32_kernel's frame: persistent
//       workgroups over 128-wide tiles, 8 outputs per thread, every tile row straight-line code
//       (Geom, for_each_row), the next tile's HBM reads in flight under the current tile's taps,
//       xcd_tile's placement, launch_c1_tiles.
//   bilateral_f32c_k1_kernel<C, FMA>   ksize 1: elementwise; the one tap has d = 0 (or NaN), so no
//       address is formed from the source, no table is read and no LDS is used.
// There is no runtime-radius kernel: ksize stops at 15.
//
// What is shared and what is not: Geom, lds_bytes / pick_waves, PairStage and the kBf32 constants,
// xcd_tile, for_each_row, set_progress_priority and launch_c1_tiles are used as they are, and the
// argument struct is BilateralF32Args as vip_bilateral_f32_run_rows fills it (a pixel of src and
// dst is C floats). The tile prefetch (Bf32cPrefetch), the row reader (Bf32cRow), the tap loop
// (bf32c_row_taps) and the store are this file's own, for the reason vip_joint_f32c.hip gives for
// its own: the shared ones name their planes one by one, and that file's N-plane forms carry a
// guide plane and StencilArgs' guide loads, which this filter does not have.
#pragma once

#include "vip_bilateral_f32.hpp"

namespace vip {

constexpr int kBf32cP = kBf32P;

// Waves per workgroup the registers hold without scratch, by channel count and radius
// (profiles/bilateral_f32c_resources.txt): 16 waves have 128 VGPRs per lane, 12 have 168, 8 have 256.
// C = 2 needs 113 to 127 at R <= 2 and 142 to 148 from R = 3; C = 3 needs 150 to 163 at R <= 2 and,
// compiled as 12 waves, all 168 and 56 to 88 bytes of scratch at R = 3 and 4 (178 to 201 as 8 waves).
template <int C, int R>
constexpr int bf32c_max_waves() {
    static_assert(C == 2 || C == 3, "channels");
    static_assert(R >= 1 && R <= kBf32cMaxRadius, "radius");
    if constexpr (C == 2) return R <= 2 ? 16 : 12;
    return R <= 2 ? 12 : 8;
}

// The wave count and the LDS bytes (the header's rule)
template <int C, int R>
struct Bf32cForm {
    static constexpr int WAVES = pick_waves<R, C, bf32c_max_waves<C, R>(), kBf32LutW, kBf32cP, 16>();
    static constexpr int LDS = lds_bytes<R, WAVES, C, kBf32LutW, kBf32cP, 16>();
    static_assert(WAVES >= 8, "8 waves fit beside the table's full 8 copies: the copies are never halved");
    static_assert(LDS <= kLdsBudget, "the planes and the pair table fit LDS");
};

// 4 pixels of one image row from column x (columns clamped to the image): the source's 4 * C
// floats in memory order (f[k * C + c]: pixel k, channel c), as loaded from HBM; channel_words(c)
// is plane c's 4 words (vip_joint_f32c.hip's F32cGroup without a guide).
template <int C>
struct Bf32cGroup {
    float f[4 * C];

    __device__ __forceinline__ void load(const BilateralF32Args& a, int sy, int x) {
        const float* frow = reinterpret_cast<const float*>(a.src + (long long)sy * a.src_pitch);
        if ((a.aligned & kF32SrcVec) && x >= 0 && x + 3 < a.width) {  // x is a multiple of 4: 16 * C bytes from a 16-byte boundary
            const float4* p = reinterpret_cast<const float4*>(frow + x * C);
#pragma unroll
            for (int q = 0; q < C; ++q) {
                const float4 v = p[q];
                f[4 * q + 0] = v.x;
                f[4 * q + 1] = v.y;
                f[4 * q + 2] = v.z;
                f[4 * q + 3] = v.w;
            }
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float* px = frow + clampi(x + k, 0, a.width - 1) * C;
#pragma unroll
                for (int c = 0; c < C; ++c) f[k * C + c] = px[c];
            }
        }
    }
    __device__ __forceinline__ uint4 channel_words(int c) const {
        return make_uint4(__float_as_uint(f[c]), __float_as_uint(f[C + c]), __float_as_uint(f[2 * C + c]),
                          __float_as_uint(f[3 * C + c]));
    }
};

// Register-staged prefetch of one tile's C planes (C1Prefetch's N-plane form): issue() starts the
// HBM loads of source rows [ty0 + src_row0 - R, +ROWS) x columns [tx0 - L, tx0 + TW + L), rows
// clamped to [row_lo, row_hi), columns to [0, width); commit() writes plane c at planes + c * PLANE.
template <int R, int ROWS, int NT, int C>
struct Bf32cPrefetch {
    using G = Geom<R, kBf32cP, 16>;
    static constexpr int NG = ROWS * G::GROUPS;
    static constexpr int K = (NG + NT - 1) / NT;
    static constexpr int PLANE = ROWS * G::S;
    Bf32cGroup<C> raw[K];

    __device__ __forceinline__ void issue(const BilateralF32Args& a, int tx0, int ty0) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int g = (int)threadIdx.x + k * NT;
            if (NG % NT != 0 && k == K - 1 && g >= NG) continue;
            const int r = g / G::GROUPS;
            const int gc = g - r * G::GROUPS;
            const int sy = clampi(ty0 + a.src_row0 - R + r, a.row_lo, a.row_hi - 1);
            raw[k].load(a, sy, tx0 - G::L + 4 * gc);
        }
    }
    __device__ __forceinline__ void commit(uint32_t* planes) const {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int g = (int)threadIdx.x + k * NT;
            if (NG % NT != 0 && k == K - 1 && g >= NG) continue;
            const int r = g / G::GROUPS;
            const int gc = g - r * G::GROUPS;
            uint32_t* const p = planes + r * G::S + 4 * gc;
#pragma unroll
            for (int c = 0; c < C; ++c) *reinterpret_cast<uint4*>(p + c * PLANE) = raw[k].channel_words(c);
        }
    }
};

// Neighbour words of one tile row of the C planes, columns [4 * C0, 4 * C0 + 4 * NC), read chunk by
// chunk (RowStream's N-plane form; volatile for the reason given there). PLANE4: uint4s between
// two planes.
template <int C0, int NC, int C, int PLANE4>
struct Bf32cRow {
    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
    typedef __attribute__((address_space(3))) const volatile u32x4 lds_u32x4;
    lds_u32x4* g;
    float fw[C][4 * NC];

    __device__ __forceinline__ Bf32cRow(const uint32_t* planes, int row_off)
        : g((lds_u32x4*)(planes) + (row_off >> 2) + C0) {}

    __device__ __forceinline__ void load(int q) {
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const u32x4 u = g[q + c * PLANE4];
            fw[c][4 * q + 0] = __uint_as_float(u.x); fw[c][4 * q + 1] = __uint_as_float(u.y);
            fw[c][4 * q + 2] = __uint_as_float(u.z); fw[c][4 * q + 3] = __uint_as_float(u.w);
        }
    }
};

// The tap loop of one tile row (bf32_row_taps with C sums): neighbour column j serves output i at
// kx = j - L - i, per output the taps run in ascending kx, the pair reads kPipeDepth columns ahead
// of their use; distance, index, pair read, interpolation and ws * wc once per tap, then C fmas and
// sumk's add. cf: the outputs' centre values per channel; lane8: 8 * the lane's table copy.
template <int HW, int L, int C0, int NC, bool FMA, int P, int C, int PLANE4>
__device__ __forceinline__ void bf32c_row_taps(const uint32_t* planes, int row_off, const float (&wsv)[HW + 1],
                                               const char* lut, uint32_t lane8, float scale,
                                               const float (&cf)[C][P], float (&s)[C][P], float (&sk)[P]) {
    constexpr int D = kPipeDepth, NB = D + 1;
    constexpr int J0 = L - HW, J1 = L + P - 1 + HW;
    constexpr int LA = D + kRowLookahead;
    static_assert(J0 >= 4 * C0 && J1 < 4 * (C0 + NC), "row chunk range");
    auto chunk = [](int j) constexpr { return (j - 4 * C0) >> 2; };
    constexpr int PRE = chunk(J0 + LA < J1 ? J0 + LA : J1);
    Bf32cRow<C0, NC, C, PLANE4> row(planes, row_off);
#pragma unroll
    for (int q = 0; q <= PRE; ++q) row.load(q);
    float2 pr[NB][P];
    float av[NB][P];
    auto issue = [&](int j) {
        const int b = (j - J0) % NB;
#pragma unroll
        for (int i = 0; i < P; ++i) {
            const int kx = j - L - i;
            if (kx < -HW || kx > HW) continue;
            float d = __builtin_fabsf(row.fw[0][j - 4 * C0] - cf[0][i]) + __builtin_fabsf(row.fw[1][j - 4 * C0] - cf[1][i]);
            if constexpr (C == 3) d = d + __builtin_fabsf(row.fw[2][j - 4 * C0] - cf[2][i]);
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
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const float nf = row.fw[c][j - 4 * C0];
                if constexpr (FMA)
                    s[c][i] = __builtin_fmaf(nf, w, s[c][i]);
                else
                    s[c][i] = s[c][i] + nf * w;
            }
            sk[i] = sk[i] + w;
        }
        __builtin_amdgcn_sched_barrier(0);
    }
}

// Write the C channels of P outputs of row oy from column x (a multiple of P), interleaved:
// P * C consecutive floats, as 16-byte stores where dst allows them (dst_aligned: base and pitch
// are 16-byte aligned; P * C * 4 is a multiple of 32) and the outputs are all inside the row,
// single dwords otherwise; never a byte at column >= width or row >= out_rows
// (vip_joint_f32c.hip's store on this kernel's arguments).
template <int C, int P>
__device__ __forceinline__ void store_bf32c(const BilateralF32Args& a, int oy, int x, const float (&o)[C][P]) {
    if (oy >= a.out_rows || x >= a.width) return;
    float* p = reinterpret_cast<float*>(a.dst + (long long)oy * a.dst_pitch) + x * C;
    if (a.dst_aligned && x + P <= a.width) {
#pragma unroll
        for (int q = 0; q < P * C / 4; ++q) {
            const int e = 4 * q;  // element e is channel e % C of output e / C
            reinterpret_cast<float4*>(p)[q] = make_float4(o[e % C][e / C], o[(e + 1) % C][(e + 1) / C],
                                                          o[(e + 2) % C][(e + 2) / C], o[(e + 3) % C][(e + 3) / C]);
        }
        return;
    }
#pragma unroll
    for (int i = 0; i < P; ++i)
        if (x + i < a.width) {
#pragma unroll
            for (int c = 0; c < C; ++c) p[i * C + c] = o[c][i];
        }
}

template <int R, int C, bool FMA>
__global__ __launch_bounds__((Bf32cForm<C, R>::WAVES * 64)) void bilateral_f32c_kernel(const BilateralF32Args a) {
    using W = Bf32cForm<C, R>;
    constexpr int P = kBf32cP, WAVES = W::WAVES, NT = WAVES * 64;
    using G = Geom<R, P, 16>;
    constexpr int TH = WAVES * G::RPW;
    constexpr int ROWS = TH + 2 * R;
    constexpr int PLANE = ROWS * G::S;
    static_assert(4 * (kBf32LutW + C * PLANE) == W::LDS, "the planes and the pair table are the launch's LDS bytes");
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    uint32_t* const lut = lds;
    uint32_t* const planes = lds + kBf32LutW;  // f_0 .. f_{C-1}
    static_assert(kBf32LutW % 4 == 0, "the planes start 16-byte aligned");

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tx = lane & 15;
    const int ty = wave * G::RPW + (lane >> 4);
    static_assert(G::S % 4 == 0 && P % 4 == 0 && PLANE % 4 == 0, "plane rows in uint4");
    const int base4 = ty * (G::S / 4) + tx * (P / 4);  // uint4 index of the thread's tile row, column tx * P
    const uint32_t lane8 = (uint32_t)(lane & (kBf32Copies - 1)) << 3;  // this lane's table copy
    const char* const lut_bytes = reinterpret_cast<const char*>(lut);
    const float scale = a.scale;

    // persistent: workgroup b filters tiles b, b + grid, ... (xcd_tile's placement)
    int tile = blockIdx.x;
    Bf32cPrefetch<R, ROWS, NT, C> pf;
    PairStage<NT> ls;
    ls.load(a.color);
    {
        const int t = xcd_tile(tile, a.tiles_total);
        pf.issue(a, (t % a.tiles_x) * G::TW, (t / a.tiles_x) * TH);
    }
    ls.store(lut);
    pf.commit(planes);
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
            float cf[C][P];  // the outputs' centre values, held across the tile row
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const uint4* ctr = reinterpret_cast<const uint4*>(planes + c * PLANE + (ty + R) * G::S + tx * P + G::L);
#pragma unroll
                for (int q = 0; q < P / 4; ++q) {
                    const uint4 v = ctr[q];
                    cf[c][4 * q + 0] = __uint_as_float(v.x);
                    cf[c][4 * q + 1] = __uint_as_float(v.y);
                    cf[c][4 * q + 2] = __uint_as_float(v.z);
                    cf[c][4 * q + 3] = __uint_as_float(v.w);
                }
            }
            float s[C][P], sk[P];
#pragma unroll
            for (int i = 0; i < P; ++i) {
                sk[i] = 0.f;
#pragma unroll
                for (int c = 0; c < C; ++c) s[c][i] = 0.f;
            }

            for_each_row<R, true>([&](const int ky, auto hwc) {
                // as bilateral_f32_kernel: every row of a plane is one base register plus a ds_read immediate
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
                bf32c_row_taps<HW, G::L, C0, NC, FMA, P, C, PLANE / 4>(planes, row_off, wsv, lut_bytes, lane8, scale, cf,
                                                                       s, sk);
                // pin the accumulators at the row's end (fence_accumulators)
#pragma unroll
                for (int i = 0; i < P; ++i) {
                    __asm__ volatile("" : "+v"(sk[i]));
#pragma unroll
                    for (int c = 0; c < C; ++c) __asm__ volatile("" : "+v"(s[c][i]));
                }
            });

#pragma unroll
            for (int i = 0; i < P; ++i)
#pragma unroll
                for (int c = 0; c < C; ++c) s[c][i] = s[c][i] / sk[i];
            store_bf32c<C, P>(a, ty0 + ty, tx0 + tx * P, s);
        }
        if (next >= a.tiles_total) break;
        __syncthreads();  // every wave is done reading this tile
        pf.commit(planes);
        __syncthreads();
        tile = next;
    }
}

// ksize 1: the one tap has d = 0 whenever the pixel is finite, so t = 0, a = 0 and
// wc = fmaf(0, D[0], L[0]) = L[0] + 0 * D[0] = L[0] (D[0] is finite); w = ws[0,0] * L[0] = 1,
// s_c = fmaf(f_c, w, 0) (0 + f_c * w in the CPP profile) and sumk = 0 + w. No address is formed from
// the source. A row is width * C floats, one per thread; the band as bilateral_f32_kernel<0>.
constexpr int kBf32cK1Threads = 256;
constexpr int kBf32cK1MaxGridY = 65535;  // rows beyond it stride over grid.y
template <int C, bool FMA>
__global__ __launch_bounds__(kBf32cK1Threads) void bilateral_f32c_k1_kernel(const BilateralF32Args a) {
    const int e = (int)(blockIdx.x * kBf32cK1Threads + threadIdx.x);
    if (e >= a.width * C) return;
    const float w = a.ws[0] * a.color[0];
    const float sk = 0.f + w;
    for (int y = (int)blockIdx.y; y < a.out_rows; y += (int)gridDim.y) {
        const int sy = clampi(y + a.src_row0, a.row_lo, a.row_hi - 1);
        const float f = reinterpret_cast<const float*>(a.src + (long long)sy * a.src_pitch)[e];
        float s;
        if constexpr (FMA)
            s = __builtin_fmaf(f, w, 0.f);
        else
            s = 0.f + f * w;
        reinterpret_cast<float*>(a.dst + (long long)y * a.dst_pitch)[e] = s / sk;
    }
}

template <int C, bool FMA>
static int launch_bf32c_k1(const BilateralF32Args& a, hipStream_t stream) {
    note_launch(reinterpret_cast<const void*>(bilateral_f32c_k1_kernel<C, FMA>));
    if (a.width <= 0 || a.out_rows <= 0) return 0;
    const dim3 grid((unsigned)((a.width * C + kBf32cK1Threads - 1) / kBf32cK1Threads),
                    (unsigned)(a.out_rows < kBf32cK1MaxGridY ? a.out_rows : kBf32cK1MaxGridY));
    launch(bilateral_f32c_k1_kernel<C, FMA>, grid, dim3(kBf32cK1Threads), 0u, stream, a);
    return (int)hipGetLastError();
}

// The kernels are instantiated by four small units, vip_bilateral_f32c_c2_fma.hip .. _c3_mul.hip, one
// per channel count and arithmetic, which build in parallel (the straight-line tile rows make the
// compiler's time grow with the square of the tap count, as in vip_bilateral_f32.hpp); each
// instantiates launch_bilateral_f32c_unit (vip_launch.hpp) for its pair, radius 0..kBf32cMaxRadius.
template <int C, bool FMA>
int launch_bilateral_f32c_unit(int radius, const BilateralF32Args& a, hipStream_t stream) {
    if (radius == 0) return launch_bf32c_k1<C, FMA>(a, stream);
    int rc = VIP_ERR_UNSUPPORTED_KSIZE;
    [&]<int... I>(std::integer_sequence<int, I...>) {
        (void)(... || (radius == I + 1 && (rc = [&] {
                           constexpr int R = I + 1;
                           using W = Bf32cForm<C, R>;
                           return launch_c1_tiles<bilateral_f32c_kernel<R, C, FMA>, W::LDS, W::WAVES,
                                                  Geom<R, kBf32cP, 16>>(a, stream);
                       }(), true)));
    }(std::make_integer_sequence<int, kBf32cMaxRadius>{});
    return rc;
}

}  // namespace vip
