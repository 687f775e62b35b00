// Single-channel (8-bit gray) bilateral and joint-bilateral kernels for gfx950 (MI355X).
//
// Definition (include/vip.h, vip_bilateral_run_c1): per output pixel and per tap in row-major
// order over the k x k square, w = ws[ky,kx] * wc[d], s += g_n * w, sumk += w,
// dst = u8(s / sumk + 0.5f), replicate border; d = |g_n - g_c| (plain), |G_n - G_c| (gray
// guide G) or |dB| + |dG| + |dR| (3-channel guide). That is channel 0 of the 3-channel
// filter on the frame (g, 0, 0), so the 3-channel oracle is this one's oracle.
//
// One LDS word per pixel in every form, so one ds_read_b128 feeds 4 neighbours and
// v_sad_u8 yields the colour distance in one instruction:
//   plain        word = g                       d = sad(word, centre)
//   gray guide   word = G | g << 8              d = sad(word & 0xff, centre)
//   RGB guide    word = B | G << 8 | R << 16 | g << 24   d = sad(word & 0xffffff, centre)
// The mask and the u8 -> float conversion of g are per neighbour word, shared by the
// thread's outputs; a tap is v_sad_u8, v_lshl_add (LUT address), ds_read_b32, v_mul (spatial
// weight from an SGPR), v_fmac, v_add: 5 VALU against the 3-channel kernel's 7 (counted in the
// radius-7 kernel's assembly: 1192 of each per thread and tile, 5.6 VALU per tap overall).
// The colour LUT is the handle's 768-entry table; the plain and gray-guide forms reach only
// its first 256 entries and hold 256 x 32 interleaved copies (32 KiB), the RGB-guide form
// 768 x 32 (96 KiB).
//
// Two kernels, as for the 3-channel filters:
//   gray_kernel<R, GUIDE, FMA>     radius 1..15 a template argument; persistent 16-wave
//       workgroups over 128 x 64 tiles, 8 outputs per thread, every tile row straight-line
//       code with a compile-time disc half-width (vip_stencil.hpp: Geom, for_each_row,
//       RowStream), the next tile's HBM reads in flight under the current tile's taps.
//   gray_rt_kernel<GUIDE, FMA>     radius a kernel argument (0 and 16..32, or every radius
//       under VIP_PATH_RUNTIME); one workgroup per 64 x 64 tile, 4 outputs per thread, taps
//       in blocks of 4 with exact zero weights outside the disc (as vip_stencil_rt.hip;
//       tile geometry and launch: vip_rt.hpp).
// The tap loop of a tile row, gray_row_taps, is vip_gray.hpp's, here with the GraySad index.
// Both numerics profiles (FMA: explicit __builtin_fmaf; otherwise mul + add, the build
// has -ffp-contract=off) are instantiated here.
#include "vip_gray.hpp"

namespace vip {

constexpr int kGrayP = 8, kGrayWaves = 16;
template <int R, int GUIDE>
constexpr int gray_lds_bytes() {
    return 4 * (GrayWord<GUIDE>::ENTRIES * kGrayCopies + (kGrayWaves * 4 + 2 * R) * Geom<R, kGrayP, 16>::S);
}

template <int R, int GUIDE, bool FMA>
__global__ __launch_bounds__(kGrayWaves * 64) void gray_kernel(const StencilArgs a) {
    using W = GrayWord<GUIDE>;
    constexpr int P = kGrayP, WAVES = kGrayWaves, NT = WAVES * 64;
    using G = Geom<R, P, 16>;
    constexpr int TH = WAVES * G::RPW;
    constexpr int ROWS = TH + 2 * R;
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    uint32_t* const lut = lds;
    uint32_t* const plane = lds + W::ENTRIES * kGrayCopies;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tx = lane & 15;
    const int ty = wave * G::RPW + (lane >> 4);
    const uint32_t lane4 = (uint32_t)(lane & (kGrayCopies - 1)) << 2;  // this lane's LUT copy
    const char* const lut_bytes = reinterpret_cast<const char*>(lut);

    // persistent: workgroup b filters tiles b, b + grid, ... (xcd_tile's placement)
    int tile = blockIdx.x;
    C1Prefetch<R, ROWS, NT, P, GrayGroup<GUIDE>> pf;
    LutStage<NT, W::ENTRIES, kGrayCopies> ls;
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
            GraySad<GUIDE, P> dist;
            {
                const uint4* c = reinterpret_cast<const uint4*>(plane + (ty + R) * G::S + tx * P + G::L);
#pragma unroll
                for (int q = 0; q < P / 4; ++q) {
                    const uint4 v = c[q];
                    dist.ctr[4 * q + 0] = W::guide(v.x);
                    dist.ctr[4 * q + 1] = W::guide(v.y);
                    dist.ctr[4 * q + 2] = W::guide(v.z);
                    dist.ctr[4 * q + 3] = W::guide(v.w);
                }
            }
            float s[P], sk[P];
#pragma unroll
            for (int i = 0; i < P; ++i) s[i] = sk[i] = 0.f;

            for_each_row<R, true>([&](const int ky, auto hwc) {
                const int row_off = (ty + R + ky) * G::S + tx * P;
                gray_tile_row<R, decltype(hwc)::value, G::L, FMA>(a, ky, plane, row_off, lut_bytes, lane4, dist, s, sk);
            });

            uint32_t o[P];
#pragma unroll
            for (int i = 0; i < P; ++i) o[i] = f2u8(s[i] / sk[i] + 0.5f);
            store_gray(a, ty0 + ty, tx0 + tx * P, o);
        }
        if (next >= a.tiles_total) break;
        __syncthreads();  // every wave is done reading this tile
        pf.commit(plane);
        __syncthreads();
        tile = next;
    }
}

template <int GUIDE, bool FMA>
static int launch_gray_dispatch(int radius, const StencilArgs& a, hipStream_t stream) {
    return dispatch_radius(radius, [&](auto rc) {
        constexpr int R = decltype(rc)::value;
        return launch_c1_tiles<gray_kernel<R, GUIDE, FMA>, gray_lds_bytes<R, GUIDE>(), kGrayWaves,
                               Geom<R, kGrayP, 16>>(a, stream);
    });
}

int launch_gray(int radius, int guide_channels, bool fma, const StencilArgs& a, hipStream_t s) {
    switch (guide_channels) {
        case 0: return fma ? launch_gray_dispatch<0, true>(radius, a, s) : launch_gray_dispatch<0, false>(radius, a, s);
        case 1: return fma ? launch_gray_dispatch<1, true>(radius, a, s) : launch_gray_dispatch<1, false>(radius, a, s);
        case 3: return fma ? launch_gray_dispatch<3, true>(radius, a, s) : launch_gray_dispatch<3, false>(radius, a, s);
        default: return VIP_ERR_INVALID_ARGUMENT;
    }
}

// ---------------------------------------------------------------- runtime radius
// 4 consecutive plane words: guide bytes (colour distance) and source floats (sums)
template <int GUIDE>
struct GrayRtWin {
    uint32_t g[4];
    float c[4];
    __device__ __forceinline__ void load(const uint32_t* plane, int off) {
        const uint4 v = *reinterpret_cast<const uint4*>(plane + off);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            g[k] = GrayWord<GUIDE>::guide(w[k]);
            c[k] = GrayWord<GUIDE>::source(w[k]);
        }
    }
};

template <int GUIDE, bool FMA>
__global__ __launch_bounds__(kRtWaves * 64) void gray_rt_kernel(const RtArgs a) {
    using W = GrayWord<GUIDE>;
    constexpr int P = kRtP, NT = kRtWaves * 64, TH = kRtWaves * 4;
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const int R = a.R, L = a.L, S = a.S;
    const int rows = TH + 2 * R;
    const int pw = rt_plane_words(R, L, S);
    uint32_t* const plane = lds;
    uint32_t* const lut = lds + pw;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tx = lane & 15;
    const int ty = wave * 4 + (lane >> 4);
    const int tile = blockIdx.x;
    const int tx0 = (tile % a.tiles_x) * kRtTW, ty0 = (tile / a.tiles_x) * TH;

    // colour LUT: word d * 32 + c = color[d]
    for (int q = tid; q < W::ENTRIES * kGrayCopies / 4; q += NT) {
        const uint32_t v = __float_as_uint(a.color[q >> 3]);
        *reinterpret_cast<uint4*>(lut + 4 * q) = make_uint4(v, v, v, v);
    }
    // tile plane; columns [TW + 2L, S) and the pad are zeroed: the last tap block of a row
    // reads up to 4 words past its apron (weight 0), and a zero word's distance to any
    // centre stays inside the LUT (d <= 255, or 765 with a 3-channel guide)
    {
        const int gpr = S / 4, valid = (kRtTW + 2 * L) / 4;
        for (int q = tid; q < rows * gpr; q += NT) {
            const int r = q / gpr, gc = q - r * gpr;
            uint4 w = make_uint4(0u, 0u, 0u, 0u);
            if (gc < valid) {
                const int sy = clampi(ty0 + a.src_row0 - R + r, a.row_lo, a.row_hi - 1);
                GrayGroup<GUIDE> grp;
                grp.load(a.src, a.src_pitch, a.guide, a.guide_pitch, sy, tx0 - L + 4 * gc, a.width, a.aligned);
                w = grp.words();
            }
            *reinterpret_cast<uint4*>(plane + r * S + 4 * gc) = w;
        }
        if (L < 4 && tid < 2) *reinterpret_cast<uint4*>(plane + rows * S + 4 * tid) = make_uint4(0u, 0u, 0u, 0u);
    }
    __syncthreads();
    if (ty0 + wave * 4 >= a.out_rows) return;  // wave-uniform; no barrier follows

    const int xc = L + tx * P;  // plane column of the thread's output 0
    uint32_t ctr[P];
    {
        const uint4 v = *reinterpret_cast<const uint4*>(plane + (ty + R) * S + xc);
        ctr[0] = W::guide(v.x); ctr[1] = W::guide(v.y); ctr[2] = W::guide(v.z); ctr[3] = W::guide(v.w);
    }
    const uint32_t lanec = (uint32_t)(lane & (kGrayCopies - 1)) << 2;
    const char* const lut_bytes = reinterpret_cast<const char*>(lut);

    float s[P], sk[P];
#pragma unroll
    for (int i = 0; i < P; ++i) s[i] = sk[i] = 0.f;

    // 4 taps x 4 outputs: tap t of the block pairs output i with word t + i of cur|nxt
    auto block = [&](const GrayRtWin<GUIDE>& cur, const GrayRtWin<GUIDE>& nxt, const kconst float* wsb) {
        const float wsv[4] = {wsb[0], wsb[1], wsb[2], wsb[3]};  // uniform: one scalar load
        float wc[4][P];
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int i = 0; i < P; ++i) {
                const int j = t + i;
                const uint32_t d = __builtin_amdgcn_sad_u8(j < 4 ? cur.g[j & 3] : nxt.g[j & 3], ctr[i], 0u);
                wc[t][i] = *reinterpret_cast<const float*>(lut_bytes + ((d << 7) | lanec));
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
        GrayRtWin<GUIDE> A, B;
        A.load(plane, off);
        int b = 0;
        for (; b + 2 <= nblk; b += 2) {  // two blocks per trip: the windows swap roles
            B.load(plane, off + 4 * (b + 1));
            block(A, B, wsr + 4 * b);
            A.load(plane, off + 4 * (b + 2));
            block(B, A, wsr + 4 * (b + 1));
        }
        if (b < nblk) {
            B.load(plane, off + 4 * (b + 1));
            block(A, B, wsr + 4 * b);
        }
    }

    uint32_t o[P];
#pragma unroll
    for (int i = 0; i < P; ++i) o[i] = f2u8(s[i] / sk[i] + 0.5f);
    store_gray(a, ty0 + ty, tx0 + tx * P, o);
}

template <int GUIDE, bool FMA>
static int launch_gray_rt_g(RtArgs a, hipStream_t stream) {
    if (const int rc = rt_prepare(a)) return rc;
    const long long lds = 4LL * (rt_plane_words(a.R, a.L, a.S) + GrayWord<GUIDE>::ENTRIES * kGrayCopies);
    return launch_rt_tiles<gray_rt_kernel<GUIDE, FMA>>(a, lds, stream);
}

int launch_gray_rt(const RtArgs& a, int guide_channels, bool fma, hipStream_t s) {
    switch (guide_channels) {
        case 0: return fma ? launch_gray_rt_g<0, true>(a, s) : launch_gray_rt_g<0, false>(a, s);
        case 1: return fma ? launch_gray_rt_g<1, true>(a, s) : launch_gray_rt_g<1, false>(a, s);
        case 3: return fma ? launch_gray_rt_g<3, true>(a, s) : launch_gray_rt_g<3, false>(a, s);
        default: return VIP_ERR_INVALID_ARGUMENT;
    }
}

}  // namespace vip
