// Fused guide stage of one bilateral-texture iteration on a one-channel (8-bit gray) frame,
// gfx950 (MI355X): X (u8) -> G (u8). The one-channel texture filter is the restriction of the
// 3-channel one to frames with three equal channels (include/vip.h, vip_texture_run_c1): every
// value below is what texture_guide_fused_kernel (vip_texture.hip) computes on (g, g, g), one
// channel of it, bit for bit.
//   magnitude : sqrtf((float)(3 (h^2 + v^2))), the exact integer sum of the three equal
//               channels' squares (NOT sqrt(3) times the one-channel magnitude)
//   intensity : (3 g) / 3.f == (float)g for every byte g, so the extremes of the window are
//               the integer max and min of g
//   blurred   : (float)(sum g) / ksize^2, one plane
//   rtv, argmin, alpha and the blend: as the 3-channel stage, on that one plane
//
// Regions around the output tile T, R = ksize/2, each stored PRE-CLAMPED (entry q holds the
// stage's value at clamp(q)), as in vip_texture.hip:
//   XB : image pixels as bytes, T (+) (2R+1) (origin 4-px aligned: a 4-pixel group is one
//        dword from HBM and one dword in LDS)
//   MR : gradient magnitude, T (+) 2R. XB is a quarter of the 3-channel XR, so MR has its own
//        words: the gradients go straight to LDS (none waits in registers, one barrier less)
//   H  : horizontal window aggregates of the image rows of T (+) 2R at the blur columns of
//        T (+) R, ONE word per position: sum | max << 16 | (255 - min) << 24 (the 3-channel
//        stage needs 2.5 words)
//   BR, RR : blurred and rtv, T (+) R, one plane each (alias MR/H once those are consumed)
//   GT : the guide tile as bytes (aliases XB), leaves as dwords where the guide rows allow
#include "vip_gray.hpp"
#include "vip_texture_tile.hpp"

namespace vip {

// The tile and workgroup of radius R are the 3-channel stage's (gf_tile): the phases keep its
// per-thread runs (8 pass-1 columns, 4 pass-2 rows, 4 guide rows), so its thread counts fill
// the same way; the LDS per tile is about half. Chosen from the compiler's resource report
// (DESIGN.md section 4 has the table), not from a measurement:
//   R = 4 keeps the 64-VGPR cap (63 used, nothing spilled: two 1024-thread workgroups per CU);
//   R = 7 does not take the capped 60 x 36 / 1024 tile: capped it spills 39 VGPRs (160 B of
//   scratch per lane, more than the 3-channel stage's 148 B), uncapped its 1024 threads
//   leave one workgroup per CU. It takes the 64 x 16 / 256 tile of the other large radii,
//   uncapped, without scratch.
constexpr GfTile gg_tile(int R) { return R == 7 ? GfTile{64, 16, 256} : gf_tile(R); }
constexpr int gg_min_waves(int R) { return R == 4 ? 8 : 1; }
template <int R, int TW_, int TH_, int NT_>
struct GgGeomT {
    static constexpr int TW = TW_, TH = TH_, NT = NT_;
    static_assert(TW % 4 == 0 && TH % 4 == 0, "guide tile: 4-pixel groups, 4-row runs");
    static constexpr int K = 2 * R + 1;
    static constexpr int BW = TW + 2 * R;               // BR/RR: T (+) R
    static constexpr int BH = TH + 2 * R;
    static constexpr int BHP = round_up(BH, kGfV2);     // + pass-2 overhang rows
    static constexpr int HWP = round_up(BW, kGfH1);     // H: blur columns, rows of T (+) 2R
    static constexpr int HH = BHP + 2 * R;
    static constexpr int MW = round_up(BW + 2 * R, 4);  // MR: T (+) 2R
    static constexpr int MH = HH;
    static constexpr int XL = round_up(2 * R + 1, 4);   // XB left apron (4-px aligned origin)
    static constexpr int XW = round_up(cmax(MW - 2 * R + XL + 1, HWP + XL), 4);  // bytes per XB row
    static constexpr int XH = MH + 2;
    static constexpr int XWW = XW / 4;                  // words per XB row
    static constexpr int XB_WORDS = round_up(XWW * XH, 4);
    static constexpr int MR_WORDS = MW * MH;
    static constexpr int HPL = HWP * HH;                // the H plane
    static constexpr int BPL = BW * BHP;                // one BR/RR plane
    static_assert(TW * TH <= 4 * XWW * XH, "GT reuses the XB region");
    static_assert(MR_WORDS % 4 == 0, "H rows are stored as b128");
    // XB (later GT), then MR and H (later BR and RR), then the exp table (64 doubles)
    static constexpr int ETAB = round_up(XB_WORDS + cmax(MR_WORDS + HPL, 2 * BPL), 4);
    static constexpr int WORDS_ALL = ETAB + 128;
    static constexpr int NR1 = HH * (HWP / kGfH1);      // pass-1 runs
    static constexpr int NR2 = BW * (BHP / kGfV2);      // pass-2 runs
    static constexpr int IT2 = (NR2 + NT - 1) / NT;
};
template <int R>
using GgGeom = GgGeomT<R, gg_tile(R).tw, gg_tile(R).th, gg_tile(R).nt>;

// Row bands as the 3-channel launcher takes them: rows [lo, hi) of img are the valid frame rows
// (every read clamps into them), guide rows [gy0, gy1) are produced. img: any base address,
// any pitch. `aligned` bit 0: image rows dword-aligned (dword tile loads); bit 1: guide rows
// (dword stores).
template <int R, bool CPP>
__global__ __launch_bounds__(GgGeom<R>::NT) __attribute__((amdgpu_waves_per_eu(gg_min_waves(R))))
void gray_texture_guide_kernel(const uint8_t* __restrict__ img, long long img_pitch, uint8_t* __restrict__ guide,
                               long long guide_pitch, int width, int lo, int hi, int gy0, int gy1, int ksize,
                               int aligned) {
    using G = GgGeom<R>;
    constexpr int K = G::K;  // window width; the reference divides by ksize^2 and
                             // uses sigma_alpha = 1/(5 ksize) even when ksize is even
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    uint32_t* const XBw = lds;
    const uint8_t* const XB = reinterpret_cast<const uint8_t*>(lds);
    float* const MR = reinterpret_cast<float*>(lds + G::XB_WORDS);
    uint32_t* const H = lds + G::XB_WORDS + G::MR_WORDS;
    float* const BR = reinterpret_cast<float*>(lds + G::XB_WORDS);  // aliases MR/H
    float* const RR = BR + G::BPL;
    uint8_t* const GT = reinterpret_cast<uint8_t*>(lds);            // aliases XB
    double* const etab = reinterpret_cast<double*>(lds + G::ETAB);  // kExp2Tab64
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * G::TW, y0 = gy0 + blockIdx.y * G::TH;
    // region origins (image coordinates)
    const int xr0 = x0 - G::XL, yr0 = y0 - 2 * R - 1;
    const int mr0x = x0 - 2 * R, mr0y = y0 - 2 * R;
    const int W1 = width - 1, H0 = lo, H1 = hi - 1;

    // 1. XB: 4-pixel groups, every load of the thread issued before any is stored (one HBM
    //    latency per tile); load_gray4 clamps the columns, the row is clamped here
    {
        constexpr int NG = G::XH * G::XWW, KG = (NG + G::NT - 1) / G::NT;
        uint32_t raw[KG];
#pragma unroll
        for (int k = 0; k < KG; ++k) {
            const int g = tid + k * G::NT;
            if (NG % G::NT != 0 && g >= NG) continue;
            const int ry = g / G::XWW, gx = g - ry * G::XWW;
            const uint8_t* row = img + (long long)clampi(yr0 + ry, H0, H1) * img_pitch;
            raw[k] = load_gray4(row, xr0 + 4 * gx, width, aligned & 1);
        }
        if (tid < 64) etab[tid] = kExp2Tab64[tid];  // read in phase 4, after several barriers
#pragma unroll
        for (int k = 0; k < KG; ++k) {
            const int g = tid + k * G::NT;
            if (NG % G::NT != 0 && g >= NG) continue;
            XBw[g] = raw[k];
        }
        __syncthreads();
    }

    // 2a. MR[q] = gradient at c = clamp(q); XB is pre-clamped, so c's neighbours are read
    //     directly. 3 (h^2 + v^2) is an exact integer (< 2^20), the sum the 3-channel stage
    //     forms over three equal channels.
    constexpr int NM = G::MW * G::MH, KM = (NM + G::NT - 1) / G::NT;
#pragma unroll
    for (int k = 0; k < KM; ++k) {
        set_progress_priority(k * 4 / KM);
        const int i = tid + k * G::NT;
        if (NM % G::NT != 0 && i >= NM) continue;
        const int qy = i / G::MW, qx = i - qy * G::MW;
        const int cx = clampi(mr0x + qx, 0, W1) - xr0, cy = clampi(mr0y + qy, H0, H1) - yr0;
        const uint8_t* c = XB + cy * G::XW + cx;
        const int h = (int)c[1] - (int)c[-1], v = (int)c[G::XW] - (int)c[-G::XW];
        MR[i] = sqrt_int_exact((float)(3 * (h * h + v * v)));  // == sqrtf (microbench/div_check)
    }
    // 2b. pass 1: H = horizontal K-window aggregates, kGfH1 adjacent columns per thread.
    //     H row h <-> image row y0 - 2R + h (XB row h + 1); H column c <-> image column
    //     x0 - R + c, window XB columns c + XL - 2R .. c + XL: whole dwords of the row, the
    //     bytes taken out at compile-time positions.
    for (int run = tid; run < G::NR1; run += G::NT) {
        const int hr = run / (G::HWP / kGfH1), hc0 = (run - hr * (G::HWP / kGfH1)) * kGfH1;
        constexpr int NX = kGfH1 + K - 1;
        constexpr int OFF = G::XL - 2 * R, SH = OFF % 4, NW = (SH + NX + 3) / 4;
        static_assert(kGfH1 % 4 == 0, "run origins are dword aligned");
        const uint32_t* xrow = XBw + (hr + 1) * G::XWW + (hc0 + OFF - SH) / 4;
        uint32_t w[NW];
#pragma unroll
        for (int t = 0; t < NW; ++t) w[t] = xrow[t];
        uint32_t gg[NX], mx[NX];
#pragma unroll
        for (int t = 0; t < NX; ++t) {
            gg[t] = __builtin_amdgcn_ubfe(w[(SH + t) / 4], 8 * ((SH + t) % 4), 8);
            mx[t] = ((gg[t] ^ 255u) << 16) | gg[t];  // max of lo = max g, max of hi = 255 - min g
        }
        uint32_t og[kGfH1], omx[kGfH1];
        win_sum<kGfH1, K>(gg, og);  // <= 25 * 255: 13 bits
        win_op<kGfH1, K>(mx, omx, pk_max_u16);
        uint32_t* h = H + hr * G::HWP + hc0;
#pragma unroll
        for (int j = 0; j < kGfH1; ++j) og[j] |= ((omx[j] & 0xffu) << 16) | ((omx[j] & 0xff0000u) << 8);
#pragma unroll
        for (int j = 0; j < kGfH1; j += 4)
            *reinterpret_cast<uint4*>(h + j) = make_uint4(og[j], og[j + 1], og[j + 2], og[j + 3]);
    }
    __syncthreads();
    set_progress_priority(0);

    // 3. pass 2: blur + mRTV at the BR positions, kGfV2 vertically adjacent positions per
    //    thread (vertical windows of H, magnitude sums in row-major order). Blur
    //    position (p, c) <-> image (y0 - R + p, x0 - R + c): H rows p .. p + 2R, column c;
    //    MR rows p .. p + 2R, columns c .. c + 2R. Results stay in registers until every
    //    thread is done with MR and H (BR/RR alias them).
    const float kk = (float)(ksize * ksize);
    const float rkk = 1.f / kk;
    float res[G::IT2][kGfV2][2];
#pragma unroll
    for (int it = 0; it < G::IT2; ++it) {
        const int run = tid + it * G::NT;
        if (G::NR2 % G::NT != 0 && run >= G::NR2) continue;
        const int c = run % G::BW, p0 = (run / G::BW) * kGfV2;
        const int ix = x0 - R + c, iy0 = y0 - R + p0;
        uint32_t ssum[kGfV2], smx[kGfV2];  // sum g; max g | (255 - min g) << 16
        float mmax[kGfV2], msum[kGfV2];
        if (ix >= 0 && ix <= W1 && iy0 >= H0 && iy0 + kGfV2 - 1 <= H1) {
            constexpr int NV = kGfV2 + K - 1;
            uint32_t hs[NV], hmx[NV];
            // magnitudes are finite and >= +0: their bit patterns order like their values, so
            // the extremes are integer max3s (no NaN canonicalising of LDS loads)
            uint32_t rowmax[NV], mmaxb[kGfV2];
#pragma unroll
            for (int t = 0; t < NV; ++t) {
                const uint32_t hw = H[(p0 + t) * G::HWP + c];
                hs[t] = hw & 0xffffu;
                hmx[t] = ((hw >> 16) & 0xffu) | ((hw >> 24) << 16);
            }
            win_sum<kGfV2, K>(hs, ssum);
            win_op<kGfV2, K>(hmx, smx, pk_max_u16);
#pragma unroll
            for (int t = 0; t < NV; ++t) {
                set_progress_priority(t * 4 / NV);
                const float* mrow = MR + (p0 + t) * G::MW + c;
                float m[K];
#pragma unroll
                for (int kx = 0; kx < K; ++kx) m[kx] = mrow[kx];
                uint32_t mxb = __float_as_uint(m[0]);
#pragma unroll
                for (int kx = 1; kx < K; ++kx) {  // == the reference's max (no NaN)
                    const uint32_t b = __float_as_uint(m[kx]);
                    mxb = mxb > b ? mxb : b;
                }
                rowmax[t] = mxb;
                // window row t - j of output j, in the reference's row-major order
#pragma unroll
                for (int j = 0; j < kGfV2; ++j) {
                    if (t - j < 0 || t - j >= K) continue;
                    // the reference starts from 0.f; magnitudes are >= +0, so 0.f + m == m
                    msum[j] = t == j ? m[0] : msum[j] + m[0];
#pragma unroll
                    for (int kx = 1; kx < K; ++kx) msum[j] = msum[j] + m[kx];
                }
            }
            win_op<kGfV2, K>(rowmax, mmaxb, [](uint32_t a, uint32_t b) { return a > b ? a : b; });
#pragma unroll
            for (int j = 0; j < kGfV2; ++j) mmax[j] = __uint_as_float(mmaxb[j]);
        } else {
            // a centre outside the image: the reference reads the stage values at the
            // clamped centre, whose window lies inside the pre-clamped regions
#pragma unroll
            for (int j = 0; j < kGfV2; ++j) {
                const int hrow = clampi(iy0 + j, H0, H1) - (y0 - 2 * R);  // H / MR row of the centre
                const int hcol = clampi(ix, 0, W1) - (x0 - R);            // H column; MR column hcol + R
                uint32_t as = 0, am = 0;
                float mm = 0.f, ms = 0.f;
                for (int ky = -R; ky <= R; ++ky) {
                    const uint32_t hw = H[(hrow + ky) * G::HWP + hcol];
                    as += hw & 0xffffu;
                    am = pk_max_u16(am, ((hw >> 16) & 0xffu) | ((hw >> 24) << 16));
                    const float* mrow = MR + (hrow + ky) * G::MW + hcol;
#pragma unroll
                    for (int kx = 0; kx < K; ++kx) {
                        mm = __builtin_fmaxf(mm, mrow[kx]);
                        ms = ms + mrow[kx];
                    }
                }
                ssum[j] = as;
                smx[j] = am;
                mmax[j] = mm;
                msum[j] = ms;
            }
        }
#pragma unroll
        for (int j = 0; j < kGfV2; ++j) {
            res[it][j][0] = div_exact(ssum[j], kk, rkk);
            // (3 g) / 3.f == (float)g: the intensity extremes are the byte extremes
            const float imax = (float)(smx[j] & 0xffffu);
            const float imin = (float)(255u - (smx[j] >> 16));
            const float num = (imax - imin) * mmax[j];
            res[it][j][1] = CPP ? num / (msum[j] + 1e-9f) : (float)((double)num / ((double)msum[j] + 1e-9));
        }
    }
    __syncthreads();  // MR and H are consumed: BR/RR may overwrite them
#pragma unroll
    for (int it = 0; it < G::IT2; ++it) {
        const int run = tid + it * G::NT;
        if (G::NR2 % G::NT != 0 && run >= G::NR2) continue;
        const int c = run % G::BW, p0 = (run / G::BW) * kGfV2;
#pragma unroll
        for (int j = 0; j < kGfV2; ++j) {
            const int i = (p0 + j) * G::BW + c;
            BR[i] = res[it][j][0];
            RR[i] = res[it][j][1];
        }
    }
    __syncthreads();

    // 4. guide: first strict argmin of rtv over the window (RR is pre-clamped, so the
    //    reference's clamped-coordinate scan is a direct row-major scan). A thread
    //    takes kGfRun vertically adjacent outputs: each window row's first argmin is
    //    found once and shared; scanning those rows in order with strict > then
    //    gives the row-major first argmin. Alpha blend per output, one byte into GT.
    const float sigma_alpha = 1.f / (float)(5 * ksize);
    for (int run = tid; run < (G::TH / kGfRun) * G::TW; run += G::NT) {
        const int tx = run % G::TW, ty0 = (run / G::TW) * kGfRun;
        const int x = x0 + tx;
        if (x > W1 || y0 + ty0 >= gy1) continue;
        // rtv is finite and >= +0 (num >= 0, msum + 1e-9 > 0), so its bit patterns order
        // like its values: each row's minimum is an integer min3, its first position the
        // lowest column holding that minimum -- the same position as the reference's strict >
        // scan. Every rtv is <= 255 < the scan's initial 1e10f (FLT_MAX in the CPP profile),
        // so that initial value never survives.
        uint32_t rv[kGfRun + 2 * R];
        int ri[kGfRun + 2 * R];
#pragma unroll
        for (int t = 0; t < kGfRun + 2 * R; ++t) {  // window rows ty0-R .. ty0+kGfRun-1+R
            const float* row = RR + (ty0 + t) * G::BW + tx;
            uint32_t m[K];
#pragma unroll
            for (int kx = 0; kx < K; ++kx) m[kx] = __float_as_uint(row[kx]);
            uint32_t v = m[0];
#pragma unroll
            for (int kx = 1; kx < K; ++kx) v = v < m[kx] ? v : m[kx];
            rv[t] = v;
            int c = K - 1;
#pragma unroll
            for (int kx = K - 2; kx >= 0; --kx) c = m[kx] == v ? kx : c;
            ri[t] = (ty0 + t) * G::BW + tx + c;
        }
#pragma unroll
        for (int j = 0; j < kGfRun; ++j) {
            set_progress_priority(j * 4 / kGfRun);
            const int y = y0 + ty0 + j;
            if (y >= gy1) break;
            uint32_t mb = rv[j];
#pragma unroll
            for (int ky = 1; ky < K; ++ky) mb = mb < rv[j + ky] ? mb : rv[j + ky];
            int mi = ri[j + K - 1];
#pragma unroll
            for (int ky = K - 2; ky >= 0; --ky) mi = rv[j + ky] == mb ? ri[j + ky] : mi;
            const float rmin = __uint_as_float(mb);
            const int ci = (ty0 + j + R) * G::BW + tx + R;
            const float arg = sigma_alpha * (RR[ci] - rmin);
            // == (float)exp((double)arg) for every float arg in [0, 32) (microbench/div_check)
            const float e = exp_tab_f32(arg, etab);
            // 2 / (1 + e) == 2 * RN(1 / (1 + e)) exactly; 1 + e < 2^38 (vip_texture.hip)
            const float alpha = 2.f * recip_exact(1.f + e) - 1.f;
            const float beta = 1.f - alpha;
            const float bm = BR[mi], bc = BR[ci];
            const float v = CPP ? (alpha * bm + beta * bc) + 0.5f : __builtin_fmaf(alpha, bm, beta * bc) + 0.5f;
            GT[(ty0 + j) * G::TW + tx] = (uint8_t)pack_u8_clamped(v, 0, 0u);  // == clampi((int)v, 0, 255)
        }
    }
    __syncthreads();

    // 5. guide tile -> HBM: 4 bytes -> one dword per thread (byte stores at a ragged right
    //    edge or unaligned guide rows); never a byte at column >= width or row >= gy1
    for (int q = tid; q < G::TH * (G::TW / 4); q += G::NT) {
        const int gr = q / (G::TW / 4), gx = q - gr * (G::TW / 4);
        const int x = x0 + 4 * gx, y = y0 + gr;
        if (y >= gy1 || x > W1) continue;
        const uint32_t w = lds[gr * (G::TW / 4) + gx];
        uint8_t* row = guide + (long long)y * guide_pitch + x;
        if ((aligned & 2) && x + 3 <= W1) {
            *reinterpret_cast<uint32_t*>(row) = w;
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (x + i > W1) break;
                row[i] = (uint8_t)(w >> (8 * i));
            }
        }
    }
}

template <int R, bool CPP>
static int launch_gg(const uint8_t* img, long long img_pitch, uint8_t* guide, long long guide_pitch, int width, int lo,
                     int hi, int gy0, int gy1, int ksize, int aligned, hipStream_t stream) {
    using G = GgGeom<R>;
    constexpr int LDS = 4 * G::WORDS_ALL;
    static_assert(LDS <= kLdsBudget, "gray guide tile does not fit LDS");
    constexpr auto kern = gray_texture_guide_kernel<R, CPP>;
    if (const int rc = ensure_lds<kern>(LDS)) return rc;
    note_launch(reinterpret_cast<const void*>(kern));
    if (gy1 <= gy0) return 0;
    dim3 grid((width + G::TW - 1) / G::TW, (gy1 - gy0 + G::TH - 1) / G::TH);
    launch(kern, grid, dim3(G::NT), LDS, stream, img, img_pitch, guide, guide_pitch, width, lo, hi, gy0, gy1, ksize,
           aligned);
    return (int)hipGetLastError();
}

template <bool CPP>
static int launch_gg_r(int ksize, const uint8_t* img, long long img_pitch, uint8_t* guide, long long guide_pitch,
                       int width, int lo, int hi, int gy0, int gy1, int aligned, hipStream_t s) {
    switch (ksize / 2) {  // ksize 1..24
#define VIP_CASE(RR) \
    case RR: return launch_gg<RR, CPP>(img, img_pitch, guide, guide_pitch, width, lo, hi, gy0, gy1, ksize, aligned, s);
        VIP_CASE(0) VIP_CASE(1) VIP_CASE(2) VIP_CASE(3) VIP_CASE(4) VIP_CASE(5) VIP_CASE(6)
        VIP_CASE(7) VIP_CASE(8) VIP_CASE(9) VIP_CASE(10) VIP_CASE(11) VIP_CASE(12)
#undef VIP_CASE
        default: return VIP_ERR_UNSUPPORTED_KSIZE;
    }
}

int launch_gray_texture_guide_rows(const uint8_t* img, size_t img_pitch, uint8_t* guide, size_t guide_pitch, int width,
                                   int lo, int hi, int gy0, int gy1, int ksize, bool cpp, hipStream_t stream) {
    if (!img || !guide || width <= 0 || ksize < 1 || lo < 0 || lo >= hi || gy0 < lo || gy1 > hi ||
        img_pitch < (size_t)width || guide_pitch < (size_t)width)
        return VIP_ERR_INVALID_ARGUMENT;
    const int aligned = ((uintptr_t)img % 4 == 0 && img_pitch % 4 == 0 ? 1 : 0) |
                        ((uintptr_t)guide % 4 == 0 && guide_pitch % 4 == 0 ? 2 : 0);
    return cpp ? launch_gg_r<true>(ksize, img, (long long)img_pitch, guide, (long long)guide_pitch, width, lo, hi, gy0,
                                   gy1, aligned, stream)
               : launch_gg_r<false>(ksize, img, (long long)img_pitch, guide, (long long)guide_pitch, width, lo, hi, gy0,
                                    gy1, aligned, stream);
}

}  // namespace vip
