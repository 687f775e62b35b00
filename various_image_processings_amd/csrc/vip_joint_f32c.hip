// Joint bilateral filter of an interleaved f32 source of C = 2..4 channels (flow, normals, float
// colour, RGBA) under an 8-bit guide, for gfx950 (MI355X): vip_joint_f32.hip's filter on every
// channel in one launch.
//
// Definition (include/vip.h, vip_joint_bilateral_run_f32c): per output pixel and per tap in
// row-major order over the k x k square, w = ws[ky,kx] * wc[d] is formed once, then for each
// channel s_c = fmaf(f_c(n), w, s_c) (CUDA profile) or s_c + f_c(n) * w (CPP profile), and
// sumk += w once; dst_c = s_c / sumk (IEEE binary32 division); replicate border, d as in
// vip_joint_f32.hip. Channel c of the result is, bit for bit, vip_joint_bilateral_run_f32 on plane
// c: the same operations in the same order on the same values. Every weight and every LDS
// address comes from the guide. The build's -O3 -ffp-contract=off leaves the kernels in denorm
// mode 3: gradual underflow.
//
// C + 1 LDS planes of one word per pixel: the guide word, then f_0 .. f_{C-1}. One-word planes keep
// the row strides and the conflict-free ds_read_b128 groups of the one-channel kernels (Geom::S): a
// tap row reads one more ds_read_b128 per 4 neighbours and channel. The source is de-interleaved
// once per pixel, when the prefetch commits (F32cGroup::channel_words), and re-interleaved at the
// store: a thread's 8 outputs are 8 * C consecutive floats, 2 * C whole 16-byte groups where dst
// allows them. Per tap the weight costs what it costs joint_f32_kernel (v_sad_u8, the LUT
// address, ds_read_b32, v_mul, sumk's add) and each channel adds one fma.
//
// What is shared and what is not: Guide4, Geom, lds_bytes / pick_waves, LutStage / LutStage8,
// xcd_tile, for_each_row, set_progress_priority and launch_c1_tiles are used as they are, and the
// kernel's argument struct is StencilArgs as launch_joint_f32 fills it. The tile prefetch
// (F32cPrefetch), the row reader (F32cRow) and the tap loop (f32c_row_taps) are this file's own:
// C1Prefetch, RowStream and gray_row_taps name their planes one by one (plane, fplane, cplane), and
// a count of planes as a template argument there would change text that every one-channel kernel
// compiles. The tap loop is gray_row_taps' schedule (kPipeDepth, kRowLookahead, one
// sched_barrier per neighbour column) with C sums.
//
// Wave count and LUT form per (C, GUIDE, R) (F32cForm; kLdsBudget = 160 KiB, planes of 4 bytes per
// pixel, 128-pixel-wide tiles, 8 outputs per thread everywhere):
//   the full LUT (gray guide 256 x 32 copies, conflict-free; 3-channel guide 768 x 16, <= 2-way) is
//   kept while at least 8 waves fit beside the planes; where only 4 would, the copies are halved
//   (<= 2-way, or <= 4-way at 8 copies) until 8 waves fit. Why in this order: measured on the
//   three-plane sibling (vip_joint_conf.hip), halving the copies at the same wave count costs
//   about 20 %, going from 8 to 4 waves about 30 %.
//   The wave count is then the largest that LDS allows (pick_waves) and the registers hold
//   without scratch (f32c_max_waves): the accumulators are 8 * C + 8 VGPRs and the staged
//   prefetch 4 * C + 1 (gray guide) or 4 * C + 3 (3-channel guide) VGPRs per 4-pixel group, against
//   128 VGPRs per lane at 16 waves, 168 at 12 and 256 at 8.
//   profiles/joint_f32c_resources.txt has every kernel's registers, LDS and scratch (0).
//
// Kernels:
//   joint_f32c_kernel<R, C, GUIDE, FMA>   radius 1..15 (C = 2) or 1..7 (C = 3, 4): joint_f32_kernel's
//       frame: persistent workgroups, the LUT in LDS, the next tile's HBM reads in flight under
//       the current tile's taps, xcd_tile's placement.
//   joint_f32c_k1_kernel<C, FMA>          ksize 1: elementwise, no guide read.
// There is no runtime-radius kernel.
#include "vip_gray.hpp"

namespace vip {

constexpr int kF32cP = 8;
template <int C>
constexpr int f32c_max_radius() {
    static_assert(C >= 2 && C <= 4, "channels");
    return C == 2 ? 15 : 7;
}

// Waves per workgroup the registers hold without scratch, by radius. C = 2 takes the three-plane
// sibling's limits (conf_waves: its 16-wave gray kernel spills at R = 4 and its 12-wave one at
// R = 10; this kernel holds 8 more accumulators in the same frame, and its counts stand at 128 and
// 168 at those limits). C = 3 needs 159-168 VGPRs at 12 waves, so 16 waves (128) are out at every
// radius, and from R = 5 LDS allows 8 waves only; C = 4 needs 191 at R = 1, above a 12-wave
// workgroup's 168 (profiles/joint_f32c_resources.txt).
template <int C, int GUIDE, int R>
constexpr int f32c_max_waves() {
    if constexpr (C == 2) return GUIDE == 3 ? (R <= 2 ? 16 : (R <= 8 ? 12 : 8)) : (R <= 3 ? 16 : (R <= 9 ? 12 : 8));
    if constexpr (C == 3) return R <= 4 ? 12 : 8;
    return 8;
}

// The colour LUT's form and the wave count (the header's rule)
template <int C, int GUIDE, int R>
struct F32cForm {
    static_assert(GUIDE == 1 || GUIDE == 3, "guide channels");
    static constexpr int ENTRIES = GUIDE == 3 ? 768 : 256;
    static constexpr int FULL = GUIDE == 3 ? 16 : 32;
    template <int COPIES>
    static constexpr int waves_with() {
        return pick_waves<R, C + 1, f32c_max_waves<C, GUIDE, R>(), ENTRIES * COPIES, kF32cP, 16>();
    }
    static constexpr int COPIES = waves_with<FULL>() >= 8 ? FULL
                                  : (waves_with<FULL / 2>() >= 8 || FULL / 2 == 8) ? FULL / 2
                                                                                     : FULL / 4;
    static constexpr int WAVES = waves_with<COPIES>();
    static constexpr int LUT_SHIFT = COPIES == 32 ? 7 : (COPIES == 16 ? 6 : 5);  // byte address: d << LUT_SHIFT | 4 * copy
    static constexpr int LUTW = ENTRIES * COPIES;
    static constexpr int LDS = lds_bytes<R, WAVES, C + 1, LUTW, kF32cP, 16>();
    static_assert(COPIES == 8 || COPIES == 16 || COPIES == 32, "copies");
    static_assert(WAVES >= 4 && LDS <= kLdsBudget, "the planes and the LUT fit LDS");
};

// 4 pixels of one image row from column x (columns clamped to the image): the guide's 1 or 3
// dwords and the source's 4 * C floats in memory order (f[k * C + c]: pixel k, channel c), as
// loaded from HBM; words() is the guide plane's 4 words, channel_words(c) plane c's.
template <int C, int GUIDE>
struct F32cGroup {
    Guide4<GUIDE> g;
    float f[4 * C];

    __device__ __forceinline__ void load(const StencilArgs& a, int sy, int x) {
        const bool interior = x >= 0 && x + 3 < a.width;
        const float* frow = reinterpret_cast<const float*>(a.src + (long long)sy * a.src_pitch);
        if ((a.aligned & kF32SrcVec) && interior) {  // x is a multiple of 4: 16 * C bytes from a 16-byte boundary
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
        const int gwords = a.aligned & kF32GuideWords;  // as F32Group
        g.load(a.guide + (long long)sy * a.guide_pitch, x, a.width, GUIDE == 3 ? (gwords && interior) : gwords);
    }
    __device__ __forceinline__ uint4 words() const {
        if constexpr (GUIDE == 1)
            return make_uint4(g.g0 & 0xffu, (g.g0 >> 8) & 0xffu, (g.g0 >> 16) & 0xffu, g.g0 >> 24);
        return unpack_rgb4(g.g0, g.g1, g.g2);
    }
    __device__ __forceinline__ uint4 channel_words(int c) const {
        return make_uint4(__float_as_uint(f[c]), __float_as_uint(f[C + c]), __float_as_uint(f[2 * C + c]),
                          __float_as_uint(f[3 * C + c]));
    }
};

// Register-staged prefetch of one tile's C + 1 planes (C1Prefetch's N-plane form): issue() starts
// the HBM loads of source rows [ty0 - R, +ROWS) x columns [tx0 - L, tx0 + TW + L), rows clamped to
// [row_lo, row_hi), columns to [0, width); commit() writes the guide plane at `planes` and plane c
// at planes + (c + 1) * PLANE.
template <int R, int ROWS, int NT, int C, int GUIDE>
struct F32cPrefetch {
    using G = Geom<R, kF32cP, 16>;
    static constexpr int NG = ROWS * G::GROUPS;
    static constexpr int K = (NG + NT - 1) / NT;
    static constexpr int PLANE = ROWS * G::S;
    F32cGroup<C, GUIDE> raw[K];

    __device__ __forceinline__ void issue(const StencilArgs& a, int tx0, int ty0) {
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
            *reinterpret_cast<uint4*>(p) = raw[k].words();
#pragma unroll
            for (int c = 0; c < C; ++c) *reinterpret_cast<uint4*>(p + (c + 1) * PLANE) = raw[k].channel_words(c);
        }
    }
};

// Neighbour words of one tile row of the C + 1 planes, columns [4 * C0, 4 * C0 + 4 * NC), read
// chunk by chunk (RowStream's N-plane form; volatile for the reason given there). PLANE4: uint4s
// between two planes.
template <int C0, int NC, int C, int PLANE4>
struct F32cRow {
    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
    typedef __attribute__((address_space(3))) const volatile u32x4 lds_u32x4;
    lds_u32x4* g;
    uint32_t gw[4 * NC];
    float fw[C][4 * NC];

    __device__ __forceinline__ F32cRow(const uint32_t* planes, int row_off)
        : g((lds_u32x4*)(planes) + (row_off >> 2) + C0) {}

    __device__ __forceinline__ void load(int q) {
        const u32x4 v = g[q];
        gw[4 * q + 0] = v.x; gw[4 * q + 1] = v.y; gw[4 * q + 2] = v.z; gw[4 * q + 3] = v.w;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const u32x4 u = g[q + (c + 1) * PLANE4];
            fw[c][4 * q + 0] = __uint_as_float(u.x); fw[c][4 * q + 1] = __uint_as_float(u.y);
            fw[c][4 * q + 2] = __uint_as_float(u.z); fw[c][4 * q + 3] = __uint_as_float(u.w);
        }
    }
};

// The tap loop of one tile row (gray_row_taps with C sums): neighbour column j serves output i at
// kx = j - L - i; per output the taps run in ascending kx; the weight is formed once per tap.
template <int HW, int L, int C0, int NC, bool FMA, int P, int C, int PLANE4, int LUT_SHIFT>
__device__ __forceinline__ void f32c_row_taps(const uint32_t* planes, int row_off, const float (&wsv)[HW + 1],
                                              const char* lut, uint32_t lane4, const uint32_t (&ctr)[P],
                                              float (&s)[C][P], float (&sk)[P]) {
    constexpr int D = kPipeDepth, NB = D + 1;
    constexpr int J0 = L - HW, J1 = L + P - 1 + HW;
    constexpr int LA = D + kRowLookahead;
    static_assert(J0 >= 4 * C0 && J1 < 4 * (C0 + NC), "row chunk range");
    auto chunk = [](int j) constexpr { return (j - 4 * C0) >> 2; };
    constexpr int PRE = chunk(J0 + LA < J1 ? J0 + LA : J1);
    F32cRow<C0, NC, C, PLANE4> row(planes, row_off);
#pragma unroll
    for (int q = 0; q <= PRE; ++q) row.load(q);
    float wc[NB][P];
    auto issue = [&](int j) {
        const uint32_t g = row.gw[j - 4 * C0];
        const int b = (j - J0) % NB;
#pragma unroll
        for (int i = 0; i < P; ++i) {
            const int kx = j - L - i;
            if (kx < -HW || kx > HW) continue;
            const uint32_t d = __builtin_amdgcn_sad_u8(g, ctr[i], 0u);
            wc[b][i] = *reinterpret_cast<const float*>(lut + ((d << LUT_SHIFT) | lane4));
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
            const float w = wc[b][i] * wsv[kx < 0 ? -kx : kx];
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
// single dwords otherwise; never a byte at column >= width or row >= out_rows.
template <int C, int P>
__device__ __forceinline__ void store_f32c(const StencilArgs& a, int oy, int x, const float (&o)[C][P]) {
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

template <int R, int C, int GUIDE, bool FMA>
__global__ __launch_bounds__((F32cForm<C, GUIDE, R>::WAVES * 64)) void joint_f32c_kernel(const StencilArgs a) {
    using W = F32cForm<C, GUIDE, R>;
    constexpr int P = kF32cP, WAVES = W::WAVES, NT = WAVES * 64;
    using G = Geom<R, P, 16>;
    constexpr int TH = WAVES * G::RPW;
    constexpr int ROWS = TH + 2 * R;
    constexpr int PLANE = ROWS * G::S;
    static_assert(4 * (W::LUTW + (C + 1) * PLANE) == W::LDS, "the planes and the LUT are the launch's LDS bytes");
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    uint32_t* const lut = lds;
    uint32_t* const planes = lds + W::LUTW;  // the guide plane, then f_0 .. f_{C-1}

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tx = lane & 15;
    const int ty = wave * G::RPW + (lane >> 4);
    static_assert(G::S % 4 == 0 && P % 4 == 0 && PLANE % 4 == 0, "plane rows in uint4");
    const int base4 = ty * (G::S / 4) + tx * (P / 4);  // uint4 index of the thread's tile row, column tx * P
    const uint32_t lanec = (uint32_t)(lane & (W::COPIES - 1)) << 2;  // this lane's LUT copy
    const char* const lut_bytes = reinterpret_cast<const char*>(lut);

    // persistent: workgroup b filters tiles b, b + grid, ... (xcd_tile's placement)
    int tile = blockIdx.x;
    F32cPrefetch<R, ROWS, NT, C, GUIDE> pf;
    std::conditional_t<W::COPIES == 8, LutStage8<NT, W::ENTRIES>,
                       LutStage<NT, W::ENTRIES, W::COPIES == 8 ? 16 : W::COPIES>> ls;
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
        if (ty0 + wave * G::RPW < a.out_rows) {  // wave-uniform: skip rows past the frame
            uint32_t ctr[P];  // the outputs' centre guide words
            {
                const uint4* c = reinterpret_cast<const uint4*>(planes + (ty + R) * G::S + tx * P + G::L);
#pragma unroll
                for (int q = 0; q < P / 4; ++q) {
                    const uint4 v = c[q];
                    ctr[4 * q + 0] = v.x;
                    ctr[4 * q + 1] = v.y;
                    ctr[4 * q + 2] = v.z;
                    ctr[4 * q + 3] = v.w;
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
                f32c_row_taps<HW, G::L, C0, NC, FMA, P, C, PLANE / 4, W::LUT_SHIFT>(planes, row_off, wsv, lut_bytes,
                                                                                    lanec, ctr, s, sk);
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
            store_f32c<C, P>(a, ty0 + ty, tx0 + tx * P, s);
        }
        if (next >= a.tiles_total) break;
        __syncthreads();  // every wave is done reading this tile
        pf.commit(planes);
        __syncthreads();
        tile = next;
    }
}

// ksize 1: the one tap has w = ws[0,0] * wc[0], s_c = fmaf(f_c, w, 0) (0 + f_c * w in the CPP
// profile) and sumk = 0 + w; the guide is not read. A row is width * C floats, one per thread.
constexpr int kF32cK1Threads = 256;
constexpr int kF32cK1MaxGridY = 65535;  // rows beyond it stride over grid.y
template <int C, bool FMA>
__global__ __launch_bounds__(kF32cK1Threads) void joint_f32c_k1_kernel(const StencilArgs a) {
    const int e = (int)(blockIdx.x * kF32cK1Threads + threadIdx.x);
    if (e >= a.width * C) return;
    const float w = a.ws[0] * a.color[0];
    const float sk = 0.f + w;
    for (int y = (int)blockIdx.y; y < a.out_rows; y += (int)gridDim.y) {
        const float f = reinterpret_cast<const float*>(a.src + (long long)y * a.src_pitch)[e];
        float s;
        if constexpr (FMA)
            s = __builtin_fmaf(f, w, 0.f);
        else
            s = 0.f + f * w;
        reinterpret_cast<float*>(a.dst + (long long)y * a.dst_pitch)[e] = s / sk;
    }
}

template <int C, bool FMA>
static int launch_f32c_k1(const StencilArgs& a, hipStream_t stream) {
    note_launch(reinterpret_cast<const void*>(joint_f32c_k1_kernel<C, FMA>));
    if (a.width <= 0 || a.out_rows <= 0) return 0;
    const dim3 grid((unsigned)((a.width * C + kF32cK1Threads - 1) / kF32cK1Threads),
                    (unsigned)(a.out_rows < kF32cK1MaxGridY ? a.out_rows : kF32cK1MaxGridY));
    launch(joint_f32c_k1_kernel<C, FMA>, grid, dim3(kF32cK1Threads), 0u, stream, a);
    return (int)hipGetLastError();
}

template <int C, int GUIDE, bool FMA>
static int launch_joint_f32c_dispatch(int radius, const StencilArgs& a, hipStream_t stream) {
    if (radius == 0) return launch_f32c_k1<C, FMA>(a, stream);
    return dispatch_radius(radius, [&](auto rc) {
        constexpr int R = decltype(rc)::value;
        if constexpr (R > f32c_max_radius<C>()) {
            return (int)VIP_ERR_UNSUPPORTED_KSIZE;
        } else {
            using W = F32cForm<C, GUIDE, R>;
            return launch_c1_tiles<joint_f32c_kernel<R, C, GUIDE, FMA>, W::LDS, W::WAVES, Geom<R, kF32cP, 16>>(a, stream);
        }
    });
}

template <int C>
static int launch_joint_f32c_guide(int radius, int guide_channels, bool fma, const StencilArgs& a, hipStream_t s) {
    switch (guide_channels) {
        case 1:
            return fma ? launch_joint_f32c_dispatch<C, 1, true>(radius, a, s)
                       : launch_joint_f32c_dispatch<C, 1, false>(radius, a, s);
        case 3:
            return fma ? launch_joint_f32c_dispatch<C, 3, true>(radius, a, s)
                       : launch_joint_f32c_dispatch<C, 3, false>(radius, a, s);
        default: return VIP_ERR_INVALID_ARGUMENT;
    }
}

int launch_joint_f32c(int radius, int channels, int guide_channels, bool fma, const StencilArgs& a, hipStream_t s) {
    switch (channels) {
        case 2: return launch_joint_f32c_guide<2>(radius, guide_channels, fma, a, s);
        case 3: return launch_joint_f32c_guide<3>(radius, guide_channels, fma, a, s);
        case 4: return launch_joint_f32c_guide<4>(radius, guide_channels, fma, a, s);
        default: return VIP_ERR_INVALID_ARGUMENT;
    }
}

}  // namespace vip
