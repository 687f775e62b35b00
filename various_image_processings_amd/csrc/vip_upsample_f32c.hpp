// Joint bilateral upsampling of an interleaved low-resolution f32 field of C = 2..4 channels (flow,
// normals, float colour, RGBA) under an 8-bit guide, for gfx950 (MI355X): vip_upsample.hip's filter
// on every channel in one launch. The kernels and their launcher template; one translation unit
// per channel count instantiates it (vip_upsample_f32c_c2.hip, _c3, _c4: 60 kernels each, so the
// build stays parallel).
//
// Definition (include/vip.h, vip_upsample_run_f32c): vip_upsample_run_f32's, tap by tap in the
// same row-major order; the weight w = wsp * wc[d] and sumk += w are formed once per tap, then
// s_c = fmaf(f_c(n), w, s_c) (CUDA profile) or s_c + f_c(n) * w (CPP profile) once per channel;
// dst_c = sumk == 0 ? f_c(cx, cy) : s_c / sumk. Channel c of the result is, bit for bit,
// vip_upsample_run_f32 on plane c: the same operations in the same order on the same values.
// Every weight and every LDS address comes from the guides. The build's -O3 -ffp-contract=off
// leaves the kernels in denorm mode 3: gradual underflow.
//
// upsample_f32c_kernel<R, S, C, GUIDE, FMA> is upsample_f32_kernel's frame (persistent workgroups,
// the 32-copy colour LUT and the low-resolution planes in LDS, a wave-uniform row phase so that
// the spatial row comes through scalar loads, the compile-time px, Guide4 centres from global
// memory, the next tile's group and centres in flight under the current tile's taps) with:
//   LDS       C + 1 planes of one word per cell: the guide word, then f_0 .. f_{C-1}, each in
//             UpGeom's layout. One-word planes keep the row strides that make the one-channel
//             kernel's window reads conflict-free (UpGeom::LS: at S = 2 a ds_read_b128 serves lanes
//             of two plane rows at once, and only a stride of 0 mod 64 words keeps them on
//             distinct banks; interleaved cells of C words would need a stride per C and, at
//             C = 3, reads that are no whole b128). The field is de-interleaved once per cell,
//             when the prefetch commits, and re-interleaved at the store.
//   waves     16 (128 x 64 tiles) where registers and LDS allow, else 8 (128 x 32 tiles): up_c_waves.
//             The lower tile answers both limits: the 8 * (C + 1) accumulators and the
//             (C + 1) * NWL window words of a tap row pass the 128 VGPRs of a 16-wave workgroup
//             at C = 4 (from R = 1 at S = 2, from R = 3 at S = 4 and 8), and at S = 2 with the
//             3-channel guide's 96 KiB LUT four planes of 32 + 2R rows x 128 words do not fit LDS
//             from R = 1 on, while four or five of 16 + 2R rows do (R = 4, C = 4: 5 x 24 x 512 B +
//             98,304 B = 159,744 B). The LUT
//             keeps its 32 copies and the planes UpGeom's strides. Whole float windows stay in
//             registers (the one-channel kernel's reads); 4 outputs per thread, fewer LUT copies
//             and reading the float windows cell by cell were not tried.
//   taps      one weight per tap (v_sad, the LUT read, the spatial product, sumk's add) feeding C
//             fused multiply-adds.
//   prefetch  the thread's 4-cell group is 4 * C consecutive floats: C float4 loads where the
//             source allows them.
//   store     a thread's 8 outputs are 8 * C consecutive floats: 2 * C float4 stores where dst
//             allows them, dwords otherwise.
// profiles/upsample_f32c_resources.txt has every kernel's registers, LDS and scratch (0).
#pragma once

#include "vip_upsample.hpp"

namespace vip {

// Waves per workgroup (4 output rows each): 16 where the registers hold the kernel without scratch
// and the planes fit LDS beside the LUT, else 8. Registers: C = 4 at 8 waves needs 132..147 VGPRs
// at S = 2 from R = 1 on (five 12-word windows per tap row) and 126..143 at S = 4 and 8 from
// R = 3 on, above or at the edge of a 16-wave workgroup's 128; every other kernel stays below
// (profiles/upsample_f32c_resources.txt).
template <int R, int S, int C, int GUIDE, int WAVES>
constexpr int up_c_lds_bytes_at() {
    using U = UpGeom<R, S, WAVES>;
    return 4 * (up_lut_entries<GUIDE>() * kUpCopies + (C + 1) * U::ROWS * U::LS);
}
template <int R, int S, int C, int GUIDE>
constexpr int up_c_waves() {
    static_assert(C >= 2 && C <= 4, "channels");
    if (C == 4 && R >= (S == 2 ? 1 : 3)) return 8;
    return up_c_lds_bytes_at<R, S, C, GUIDE, 16>() <= kLdsBudget ? 16 : 8;
}
template <int R, int S, int C, int GUIDE>
constexpr int up_c_lds_bytes() {
    return up_c_lds_bytes_at<R, S, C, GUIDE, up_c_waves<R, S, C, GUIDE>()>();
}

// 4 cells of one low-resolution row from column x (columns clamped to the image): the guide's 1 or
// 3 dwords and the field's 4 * C floats in memory order (f[k * C + c]: cell k, channel c), as
// loaded from HBM; channel_words(c) is plane c's 4 words.
template <int C, int GUIDE>
struct UpCGroup {
    Guide4<GUIDE> g;
    float f[4 * C];

    __device__ __forceinline__ void load(const UpsampleArgs& a, int sy, int x) {
        const bool interior = x >= 0 && x + 3 < a.low_width;
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
                const float* cell = frow + clampi(x + k, 0, a.low_width - 1) * C;
#pragma unroll
                for (int c = 0; c < C; ++c) f[k * C + c] = cell[c];
            }
        }
        const int gwords = a.aligned & kF32GuideWords;  // as F32Group
        g.load(a.guide_lo + (long long)sy * a.guide_lo_pitch, x, a.low_width,
               GUIDE == 3 ? (gwords && interior) : gwords);
    }
    __device__ __forceinline__ uint4 channel_words(int c) const {
        return make_uint4(__float_as_uint(f[c]), __float_as_uint(f[C + c]), __float_as_uint(f[2 * C + c]),
                          __float_as_uint(f[3 * C + c]));
    }
};

// UpPrefetch with C float planes: the thread's 4-cell group of the C + 1 low-resolution planes and
// its 8 centre guide pixels. commit() writes the guide plane at `planes` and plane c at
// planes + (c + 1) * PLANE.
template <int R, int S, int C, int GUIDE>
struct UpCPrefetch {
    using U = UpGeom<R, S, up_c_waves<R, S, C, GUIDE>()>;
    static constexpr int PLANE = U::ROWS * U::LS;
    UpCGroup<C, GUIDE> grp;
    Guide4<GUIDE> ctr[kUpP / 4];

    __device__ __forceinline__ void issue(const UpsampleArgs& a, int tx0, int ty0, int tx, int ty) {
        const int g = (int)threadIdx.x;
        if (g < U::NG) {
            const int r = g / U::GROUPS;
            const int gc = g - r * U::GROUPS;
            grp.load(a, clampi(ty0 / S - R + r, 0, a.low_height - 1), tx0 / S - U::L + 4 * gc);
        }
        const int y = ty0 + ty < a.out_rows ? ty0 + ty : a.out_rows - 1;
        const uint8_t* const row = a.guide + (long long)y * a.guide_pitch;
#pragma unroll
        for (int q = 0; q < kUpP / 4; ++q)
            ctr[q].load(row, tx0 + tx * kUpP + 4 * q, a.width, a.aligned & kUpGuideWords);
    }
    __device__ __forceinline__ void commit(uint32_t* planes) const {
        const int g = (int)threadIdx.x;
        if (g >= U::NG) return;
        const int r = g / U::GROUPS;
        const int gc = g - r * U::GROUPS;
        uint32_t* const p = planes + r * U::LS + 4 * gc;
        const uint4 gw = up_guide_words(grp.g);
        if constexpr (U::LS % 4 == 0) {
            *reinterpret_cast<uint4*>(p) = gw;
#pragma unroll
            for (int c = 0; c < C; ++c) *reinterpret_cast<uint4*>(p + (c + 1) * PLANE) = grp.channel_words(c);
        } else {
            p[0] = gw.x; p[1] = gw.y; p[2] = gw.z; p[3] = gw.w;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const uint4 fw = grp.channel_words(c);
                uint32_t* const fp = p + (c + 1) * PLANE;
                fp[0] = fw.x; fp[1] = fw.y; fp[2] = fw.z; fp[3] = fw.w;
            }
        }
    }
    __device__ __forceinline__ void centres(uint32_t (&c)[kUpP]) const {
#pragma unroll
        for (int q = 0; q < kUpP / 4; ++q) {
            const uint4 v = up_guide_words(ctr[q]);
            c[4 * q + 0] = v.x; c[4 * q + 1] = v.y; c[4 * q + 2] = v.z; c[4 * q + 3] = v.w;
        }
    }
};

// Write the C channels of P outputs of row oy from column x (a multiple of P), interleaved:
// P * C consecutive floats, as 16-byte stores where dst allows them (dst_aligned: base and pitch
// are 16-byte aligned; P * C * 4 is a multiple of 32) and the outputs are all inside the row,
// single dwords otherwise; never a byte at column >= width or row >= out_rows.
template <int C, int P>
__device__ __forceinline__ void up_store_f32c(const UpsampleArgs& a, int oy, int x, const float (&o)[C][P]) {
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

template <int R, int S, int C, int GUIDE, bool FMA>
__global__ __launch_bounds__((up_c_waves<R, S, C, GUIDE>() * 64)) void upsample_f32c_kernel(const UpsampleArgs a) {
    constexpr int WAVES = up_c_waves<R, S, C, GUIDE>();
    using U = UpGeom<R, S, WAVES>;
    constexpr int P = kUpP, NT = WAVES * 64, ENTRIES = up_lut_entries<GUIDE>(), PLANE = U::ROWS * U::LS;
    static_assert(up_c_lds_bytes<R, S, C, GUIDE>() <= kLdsBudget, "planes and LUT do not fit LDS");
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    uint32_t* const lut = lds;
    uint32_t* const planes = lds + ENTRIES * kUpCopies;  // the guide plane, then f_0 .. f_{C-1}

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tx = lane & 15;
    const int py = wave % S;                           // the wave's row phase
    const int crow = (wave / S) * 4 + (lane >> 4);     // the thread's cell row in the tile
    const int ty = crow * S + py;
    // plane word the thread's window starts at in its own cell row (upsample_f32_kernel's)
    const int win = (crow + R) * U::LS + U::L - R - U::OFF + tx * U::NC;
    const uint32_t lanec = (uint32_t)(lane & (kUpCopies - 1)) << 2;  // this lane's LUT copy
    const char* const lut_bytes = reinterpret_cast<const char*>(lut);

    int tile = blockIdx.x;
    UpCPrefetch<R, S, C, GUIDE> pf;
    LutStage<NT, ENTRIES, kUpCopies> ls;
    ls.load(a.color);
    {
        const int t = xcd_tile(tile, a.tiles_total);
        pf.issue(a, (t % a.tiles_x) * kUpTW, (t / a.tiles_x) * U::TH, tx, ty);
    }
    ls.store(lut);
    pf.commit(planes);
    uint32_t ctr[P];
    pf.centres(ctr);
    __syncthreads();

    for (;;) {
        const int t = xcd_tile(tile, a.tiles_total);
        const int tx0 = (t % a.tiles_x) * kUpTW, ty0 = (t / a.tiles_x) * U::TH;
        const int next = tile + (int)gridDim.x;
        if (next < a.tiles_total) {  // next tile's HBM reads fly under this tile's taps
            const int n = xcd_tile(next, a.tiles_total);
            pf.issue(a, (n % a.tiles_x) * kUpTW, (n / a.tiles_x) * U::TH, tx, ty);
        }
        if (ty0 + (wave / S) * 4 * S + py < a.out_rows) {  // wave-uniform: skip rows past the frame
            float s[C][P], sk[P];
#pragma unroll
            for (int i = 0; i < P; ++i) {
                sk[i] = 0.f;
#pragma unroll
                for (int c = 0; c < C; ++c) s[c][i] = 0.f;
            }

#pragma unroll 1
            for (int ky = -R; ky <= R; ++ky) {
                // the row of the spatial table: |oy| = 2 ay + 1, uniform -> scalar loads
                const int oy = 2 * S * ky + (S - 1) - 2 * py;
                const int ay = ((oy < 0 ? -oy : oy) - 1) >> 1;
                const kconst float* const wrow = (const kconst float*)a.wsp + ay * U::NAX;
                float wsv[U::NAX];
#pragma unroll
                for (int k = 0; k < U::NAX; ++k) wsv[k] = wrow[k];
                uint32_t gw[U::NWL], fw[C][U::NWL];
                up_load_window<U::NWL, S == 2>(planes + win + ky * U::LS, gw);
#pragma unroll
                for (int c = 0; c < C; ++c)
                    up_load_window<U::NWL, S == 2>(planes + (c + 1) * PLANE + win + ky * U::LS, fw[c]);
                // cell j of the window serves output i at kx = j - R - i / S; per output the taps run
                // in ascending kx; cell j + 1's colour-LUT reads are in flight while cell j's weights
                // are accumulated (upsample_f32_kernel's pipeline)
                float wc[2][P];
                auto issue = [&](int j) {
#pragma unroll
                    for (int i = 0; i < P; ++i) {
                        const int kx = j - R - i / S;
                        if (kx < -R || kx > R) continue;
                        const uint32_t addr = up_lut_address<GUIDE>(gw[U::OFF + j], ctr[i], lanec);
                        // the LUT starts at LDS byte 0 (launch_upsample_f32c_kernel checks it): each
                        // guide form reads it as upsample_f32_kernel does
                        if constexpr (GUIDE == 1)
                            wc[j & 1][i] =
                                *reinterpret_cast<const __attribute__((address_space(3))) float*>((size_t)addr);
                        else
                            wc[j & 1][i] = *reinterpret_cast<const float*>(lut_bytes + addr);
                    }
                };
                issue(0);
#pragma unroll
                for (int j = 0; j < U::NW; ++j) {
                    if (j + 1 < U::NW) issue(j + 1);
#pragma unroll
                    for (int i = 0; i < P; ++i) {
                        const int kx = j - R - i / S;
                        if (kx < -R || kx > R) continue;
                        const int ox = 2 * S * kx + (S - 1) - 2 * (i % S);
                        const int ax = ((ox < 0 ? -ox : ox) - 1) >> 1;
                        const float w = wsv[ax] * wc[j & 1][i];  // once per tap
#pragma unroll
                        for (int c = 0; c < C; ++c) {
                            const float f = __uint_as_float(fw[c][U::OFF + j]);
                            if constexpr (FMA)
                                s[c][i] = __builtin_fmaf(f, w, s[c][i]);
                            else
                                s[c][i] = s[c][i] + f * w;
                        }
                        sk[i] = sk[i] + w;
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
            }

            // every colour weight underflowed: the nearest low-resolution sample of each channel
#pragma unroll
            for (int c = 0; c < C; ++c)
#pragma unroll
                for (int i = 0; i < P; ++i) {
                    const float n = __uint_as_float(planes[(c + 1) * PLANE + win + U::OFF + R + i / S]);
                    s[c][i] = sk[i] == 0.f ? n : s[c][i] / sk[i];
                }
            up_store_f32c<C, P>(a, ty0 + ty, tx0 + tx * P, s);
        }
        if (next >= a.tiles_total) break;
        __syncthreads();  // every wave is done reading this tile
        pf.commit(planes);
        pf.centres(ctr);
        __syncthreads();
        tile = next;
    }
}

template <int R, int S, int C, int GUIDE, bool FMA>
static int launch_upsample_f32c_kernel(UpsampleArgs a, hipStream_t stream) {
    constexpr int LDS = up_c_lds_bytes<R, S, C, GUIDE>(), WAVES = up_c_waves<R, S, C, GUIDE>(), TH = UpGeom<R, S, WAVES>::TH;
    constexpr auto KERN = upsample_f32c_kernel<R, S, C, GUIDE, FMA>;
    // with a gray guide the kernel reads its LUT at absolute LDS addresses
    if (const int rc = ensure_lds<KERN>(LDS, GUIDE == 1)) return rc;
    note_launch(reinterpret_cast<const void*>(KERN));
    a.tiles_x = (a.width + kUpTW - 1) / kUpTW;
    a.tiles_total = a.tiles_x * ((a.out_rows + TH - 1) / TH);
    if (a.tiles_total == 0) return 0;
    launch(KERN, dim3(persistent_blocks(a.tiles_total)), dim3(WAVES * 64), LDS, stream, a);
    return (int)hipGetLastError();
}

template <int S, int C, int GUIDE, bool FMA>
static int launch_upsample_f32c_radius(int radius, const UpsampleArgs& a, hipStream_t stream) {
    int rc = VIP_ERR_UNSUPPORTED_KSIZE;
    [&]<int... I>(std::integer_sequence<int, I...>) {
        (void)(... || (radius == I && (rc = launch_upsample_f32c_kernel<I, S, C, GUIDE, FMA>(a, stream), true)));
    }(std::make_integer_sequence<int, kUpMaxRadius + 1>{});
    return rc;
}

template <int C, int GUIDE, bool FMA>
static int launch_upsample_f32c_scale(int radius, int scale, const UpsampleArgs& a, hipStream_t stream) {
    switch (scale) {
        case 2: return launch_upsample_f32c_radius<2, C, GUIDE, FMA>(radius, a, stream);
        case 4: return launch_upsample_f32c_radius<4, C, GUIDE, FMA>(radius, a, stream);
        case 8: return launch_upsample_f32c_radius<8, C, GUIDE, FMA>(radius, a, stream);
        default: return VIP_ERR_INVALID_ARGUMENT;
    }
}

template <int C>
int launch_upsample_f32c_channels(int radius, int scale, int guide_channels, bool fma, const UpsampleArgs& a,
                                  hipStream_t s) {
    switch (guide_channels) {
        case 1:
            return fma ? launch_upsample_f32c_scale<C, 1, true>(radius, scale, a, s)
                       : launch_upsample_f32c_scale<C, 1, false>(radius, scale, a, s);
        case 3:
            return fma ? launch_upsample_f32c_scale<C, 3, true>(radius, scale, a, s)
                       : launch_upsample_f32c_scale<C, 3, false>(radius, scale, a, s);
        default: return VIP_ERR_INVALID_ARGUMENT;
    }
}

}  // namespace vip
