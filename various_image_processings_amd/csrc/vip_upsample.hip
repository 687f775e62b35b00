// Joint bilateral upsampling of a low-resolution f32 field under an 8-bit guide, for gfx950
// (MI355X).
//
// Definition (include/vip.h, vip_upsample_run_f32): output (x, y) of the W x H frame lies in
// low-resolution cell (cx, cy) = (x / S, y / S) at phase (px, py) = (x % S, y % S); its taps run
// in row-major order over the (2R + 1)^2 cells around (cx, cy), cell coordinates clamped to the
// w x h low-resolution image: w = wsp * wc[d], d the distance of the cell's low-resolution guide
// pixel to the output's full-resolution one, wsp the spatial weight of the offset from the
// output pixel to the cell's centre; s = fmaf(f_n, w, s) (CUDA profile) or s + f_n * w (CPP
// profile), sumk += w, dst = sumk == 0 ? f(cx, cy) : s / sumk. The build's -O3 -ffp-contract=off
// leaves the kernels in denorm mode 3: gradual underflow, as the definition.
//
// upsample_f32_kernel<R, S, GUIDE, FMA>: persistent workgroups of 16 waves over 128 x 64 output
// tiles (xcd_tile's placement), 8 consecutive outputs of one row per thread, 16 threads per row.
//   LDS      the interleaved colour LUT (32 copies of 256 or 768 entries: 32 or 96 KiB) and the
//            tile's two low-resolution planes, the guide word (G << 7, or B | G << 8 | R << 16:
//            up_lut_address) and the float: (64 / S + 2R) rows of 128 / S + 2L cells (L = R
//            rounded up to 4, so a 4-cell group of a plane row starts at a multiple of 4 cells
//            and its floats load as one float4), at a row stride chosen per scale so that a wave's reads of 4 plane rows
//            meet no bank twice (UpGeom::LS). The largest, R = 4 at S = 2: 2 x 40 rows x 128
//            words = 40,960 B beside the LUT, 139,264 B with the 3-channel one.
//   rows     wave v filters the rows of phase py = v % S: tile rows ((v / S) * 4 + q) * S + py for
//            its four 16-lane groups q. py is then wave-uniform, and so is the row |oy| of the
//            spatial table a tap row ky reads: the weights come through scalar loads.
//   taps     per tap row a thread reads the 8 / S + 2R cells under its outputs from each plane
//            once; a cell's guide word and float feed every output of the thread that has the
//            cell in its window (S outputs share each cell's offset in cells, kx). Which entry of
//            the table row a tap takes is a compile-time constant: px = i % S for output i.
//   centres  the outputs' own guide pixels come straight from the full-resolution guide
//            (Guide4), never through LDS.
//   prefetch the next tile's plane group (every thread loads at most one) and centre pixels are
//            in flight under the current tile's taps.
// The spatial table (vip_capi.hip, upload_upsample_space) is [NAX][NAX] floats, NAX = S * R +
// S / 2: entry [ay][ax] is the weight of the offset (|ox|, |oy|) = (2 ax + 1, 2 ay + 1) half
// pixels; offsets are odd, and the weight is even in each, so the s^2 x (2R + 1)^2 phase-tap
// pairs fold into it.
#include "vip_upsample.hpp"

namespace vip {

// Register-staged prefetch of one tile: the thread's 4-cell group of the two low-resolution
// planes (rows and columns clamped to the low-resolution image) and its 8 centre guide pixels
// (row and columns clamped to the frame: a thread past the frame's edge computes, and stores
// nothing).
template <int R, int S, int GUIDE>
struct UpPrefetch {
    using U = UpGeom<R, S>;
    F32Group<GUIDE> grp;
    Guide4<GUIDE> ctr[kUpP / 4];

    __device__ __forceinline__ void issue(const UpsampleArgs& a, int tx0, int ty0, int tx, int ty) {
        const int g = (int)threadIdx.x;
        if (g < U::NG) {
            const int r = g / U::GROUPS;
            const int gc = g - r * U::GROUPS;
            const int sy = clampi(ty0 / S - R + r, 0, a.low_height - 1);
            grp.load(a.src, a.src_pitch, a.guide_lo, a.guide_lo_pitch, sy, tx0 / S - U::L + 4 * gc, a.low_width,
                     a.aligned);
        }
        const int y = ty0 + ty < a.out_rows ? ty0 + ty : a.out_rows - 1;
        const uint8_t* const row = a.guide + (long long)y * a.guide_pitch;
#pragma unroll
        for (int q = 0; q < kUpP / 4; ++q)
            ctr[q].load(row, tx0 + tx * kUpP + 4 * q, a.width, a.aligned & kUpGuideWords);
    }
    __device__ __forceinline__ void commit(uint32_t* gplane, uint32_t* fplane) const {
        const int g = (int)threadIdx.x;
        if (g >= U::NG) return;
        const int r = g / U::GROUPS;
        const int gc = g - r * U::GROUPS;
        const uint4 gw = up_guide_words(grp.g), fw = grp.source_words();
        uint32_t* const gp = gplane + r * U::LS + 4 * gc;
        uint32_t* const fp = fplane + r * U::LS + 4 * gc;
        if constexpr (U::LS % 4 == 0) {
            *reinterpret_cast<uint4*>(gp) = gw;
            *reinterpret_cast<uint4*>(fp) = fw;
        } else {
            gp[0] = gw.x; gp[1] = gw.y; gp[2] = gw.z; gp[3] = gw.w;
            fp[0] = fw.x; fp[1] = fw.y; fp[2] = fw.z; fp[3] = fw.w;
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

template <int R, int S, int GUIDE, bool FMA>
__global__ __launch_bounds__(kUpWaves * 64) void upsample_f32_kernel(const UpsampleArgs a) {
    using U = UpGeom<R, S>;
    constexpr int P = kUpP, NT = kUpWaves * 64, ENTRIES = up_lut_entries<GUIDE>();
    static_assert(up_lds_bytes<R, S, GUIDE>() <= kLdsBudget, "planes and LUT do not fit LDS");
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    uint32_t* const lut = lds;
    uint32_t* const gplane = lds + ENTRIES * kUpCopies;
    uint32_t* const fplane = gplane + U::ROWS * U::LS;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tx = lane & 15;
    const int py = wave % S;                           // the wave's row phase
    const int crow = (wave / S) * 4 + (lane >> 4);     // the thread's cell row in the tile
    const int ty = crow * S + py;
    // plane word the thread's window starts at in its own cell row: OFF words before its leftmost
    // neighbour cell (kx = -R of output 0)
    const int win = (crow + R) * U::LS + U::L - R - U::OFF + tx * U::NC;
    const uint32_t lanec = (uint32_t)(lane & (kUpCopies - 1)) << 2;  // this lane's LUT copy
    const char* const lut_bytes = reinterpret_cast<const char*>(lut);

    int tile = blockIdx.x;
    UpPrefetch<R, S, GUIDE> pf;
    LutStage<NT, ENTRIES, kUpCopies> ls;
    ls.load(a.color);
    {
        const int t = xcd_tile(tile, a.tiles_total);
        pf.issue(a, (t % a.tiles_x) * kUpTW, (t / a.tiles_x) * kUpTH, tx, ty);
    }
    ls.store(lut);
    pf.commit(gplane, fplane);
    uint32_t ctr[P];
    pf.centres(ctr);
    __syncthreads();

    for (;;) {
        const int t = xcd_tile(tile, a.tiles_total);
        const int tx0 = (t % a.tiles_x) * kUpTW, ty0 = (t / a.tiles_x) * kUpTH;
        const int next = tile + (int)gridDim.x;
        if (next < a.tiles_total) {  // next tile's HBM reads fly under this tile's taps
            const int n = xcd_tile(next, a.tiles_total);
            pf.issue(a, (n % a.tiles_x) * kUpTW, (n / a.tiles_x) * kUpTH, tx, ty);
        }
        if (ty0 + (wave / S) * 4 * S + py < a.out_rows) {  // wave-uniform: skip rows past the frame
            float s[P], sk[P];
#pragma unroll
            for (int i = 0; i < P; ++i) s[i] = sk[i] = 0.f;

#pragma unroll 1
            for (int ky = -R; ky <= R; ++ky) {
                // the row of the spatial table: |oy| = 2 ay + 1, uniform -> scalar loads
                const int oy = 2 * S * ky + (S - 1) - 2 * py;
                const int ay = ((oy < 0 ? -oy : oy) - 1) >> 1;
                const kconst float* const wrow = (const kconst float*)a.wsp + ay * U::NAX;
                float wsv[U::NAX];
#pragma unroll
                for (int k = 0; k < U::NAX; ++k) wsv[k] = wrow[k];
                uint32_t gw[U::NWL], fw[U::NWL];
                up_load_window<U::NWL, S == 2>(gplane + win + ky * U::LS, gw);
                up_load_window<U::NWL, S == 2>(fplane + win + ky * U::LS, fw);
                // cell j of the window serves output i at kx = j - R - i / S; per output the taps run
                // in ascending kx. The colour-LUT reads of cell j + 1 are in flight while cell j's
                // weights are accumulated (gray_row_taps' pipeline, one column deep).
                float wc[2][P];
                auto issue = [&](int j) {
#pragma unroll
                    for (int i = 0; i < P; ++i) {
                        const int kx = j - R - i / S;
                        if (kx < -R || kx > R) continue;
                        const uint32_t addr = up_lut_address<GUIDE>(gw[U::OFF + j], ctr[i], lanec);
                        // The LUT starts at LDS byte 0 (launch_upsample_kernel checks it). Gray guide:
                        // v_sad_u16's result goes to ds_read_b32 as it stands, 4 VALU instructions
                        // per tap instead of 5 (s = 8, k = 9 at 4K: 81.9 -> 76.8 us). The 3-channel
                        // form keeps the pointer form of its siblings: the absolute one measured
                        // 2 to 4 % slower there (profiles/upsample_4k_ab.txt).
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
                    const float f = __uint_as_float(fw[U::OFF + j]);
#pragma unroll
                    for (int i = 0; i < P; ++i) {
                        const int kx = j - R - i / S;
                        if (kx < -R || kx > R) continue;
                        const int ox = 2 * S * kx + (S - 1) - 2 * (i % S);
                        const int ax = ((ox < 0 ? -ox : ox) - 1) >> 1;
                        const float w = wsv[ax] * wc[j & 1][i];
                        if constexpr (FMA)
                            s[i] = __builtin_fmaf(f, w, s[i]);
                        else
                            s[i] = s[i] + f * w;
                        sk[i] = sk[i] + w;
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
            }

            // every colour weight underflowed: the nearest low-resolution sample
            float o[P];
#pragma unroll
            for (int i = 0; i < P; ++i) {
                const float c = __uint_as_float(fplane[win + U::OFF + R + i / S]);
                o[i] = sk[i] == 0.f ? c : s[i] / sk[i];
            }
            store_f32(a, ty0 + ty, tx0 + tx * P, o);
        }
        if (next >= a.tiles_total) break;
        __syncthreads();  // every wave is done reading this tile
        pf.commit(gplane, fplane);
        pf.centres(ctr);
        __syncthreads();
        tile = next;
    }
}

template <int R, int S, int GUIDE, bool FMA>
static int launch_upsample_kernel(UpsampleArgs a, hipStream_t stream) {
    constexpr int LDS = up_lds_bytes<R, S, GUIDE>();
    constexpr auto KERN = upsample_f32_kernel<R, S, GUIDE, FMA>;
    // with a gray guide the kernel reads its LUT at absolute LDS addresses
    if (const int rc = ensure_lds<KERN>(LDS, GUIDE == 1)) return rc;
    note_launch(reinterpret_cast<const void*>(KERN));
    a.tiles_x = (a.width + kUpTW - 1) / kUpTW;
    a.tiles_total = a.tiles_x * ((a.out_rows + kUpTH - 1) / kUpTH);
    if (a.tiles_total == 0) return 0;
    launch(KERN, dim3(persistent_blocks(a.tiles_total)), dim3(kUpWaves * 64), LDS, stream, a);
    return (int)hipGetLastError();
}

template <int S, int GUIDE, bool FMA>
static int launch_upsample_radius(int radius, const UpsampleArgs& a, hipStream_t stream) {
    int rc = VIP_ERR_UNSUPPORTED_KSIZE;
    [&]<int... I>(std::integer_sequence<int, I...>) {
        (void)(... || (radius == I && (rc = launch_upsample_kernel<I, S, GUIDE, FMA>(a, stream), true)));
    }(std::make_integer_sequence<int, kUpMaxRadius + 1>{});
    return rc;
}

template <int GUIDE, bool FMA>
static int launch_upsample_scale(int radius, int scale, const UpsampleArgs& a, hipStream_t stream) {
    switch (scale) {
        case 2: return launch_upsample_radius<2, GUIDE, FMA>(radius, a, stream);
        case 4: return launch_upsample_radius<4, GUIDE, FMA>(radius, a, stream);
        case 8: return launch_upsample_radius<8, GUIDE, FMA>(radius, a, stream);
        default: return VIP_ERR_INVALID_ARGUMENT;
    }
}

int launch_upsample_f32(int radius, int scale, int guide_channels, bool fma, const UpsampleArgs& a, hipStream_t s) {
    switch (guide_channels) {
        case 1:
            return fma ? launch_upsample_scale<1, true>(radius, scale, a, s)
                       : launch_upsample_scale<1, false>(radius, scale, a, s);
        case 3:
            return fma ? launch_upsample_scale<3, true>(radius, scale, a, s)
                       : launch_upsample_scale<3, false>(radius, scale, a, s);
        default: return VIP_ERR_INVALID_ARGUMENT;
    }
}

}  // namespace vip
