// Single-channel (8-bit gray) adaptive bilateral kernels for gfx950 (MI355X).
//
// Definition (include/vip.h, vip_adaptive_run_c1): per output pixel, replicate border,
//   mean = (float)(sum of g over the full k x k square) / (float)(k * k);  o = (float)c - mean
//   per tap in row-major order over the k x k square:
//     dist = |((float)n - (float)c) - o|;  w = ws[ky,kx] * wc[(int)dist]
//     s += n * w;  sumk += w
//   dst = u8(s / sumk + 0.5f)
// That is channel 0 of the 3-channel adaptive filter on the frame (g, 0, 0) -- channels 1 and
// 2 have n = c = mean = 0 and add exact zeros to dist -- so the 3-channel oracle is this
// filter's oracle.
//
// dist = |n - 2c + mean| with n, c and mean in [0, 255], so int(dist) <= 510 for every input
// and every sigma_color: the first 512 entries of the handle's 1536-entry colour LUT as 32
// interleaved copies (64 KiB) always suffice. Each lane reads its own copy (no bank conflict)
// at (d << 7) | lane4, with neither a clamp nor a saturating address. One LDS word per pixel
// (g), so one ds_read_b128 feeds 4 neighbours; the neighbour's float is formed once per word
// and shared by the thread's outputs. Per output the thread keeps c (a float the optimiser
// cannot see through: otherwise n - c becomes an integer subtract and a conversion), o, s
// and sumk; a tap is two v_sub_f32, v_cvt_u32_f32 |.|, v_lshl_or (LUT address), ds_read_b32,
// v_mul (spatial weight from an SGPR), v_fmac, v_add. The order ((n - c) - o) is the
// reference's; c + o is not pre-added (it rounds differently).
//
// Two kernels, as for the other filters:
//   gray_adaptive_kernel<R, FMA>   radius 1..15 a template argument; gray_kernel's frame
//       (persistent 16-wave workgroups over 128 x 64 tiles, 8 outputs per thread, straight-line
//       tile rows, the next tile's HBM reads in flight under the taps). The box sums are
//       separable at every radius: cooperative vertical K-row sums of the tile's columns
//       (16 bits each, 31 * 255 < 2^16, two columns per LDS word), then a sliding K-column
//       window per thread; the mean is div_exact's correctly rounded quotient.
//   gray_adaptive_rt_kernel<FMA>   radius a kernel argument (0 and 16..31, or every radius
//       under VIP_PATH_RUNTIME); gray_rt_kernel's frame (one workgroup per 64 x 64 tile, 4
//       outputs per thread, taps in blocks of 4 with exact zero weights outside the disc),
//       per-thread sliding row sums and the IEEE quotient as stencil_rt_kernel's adaptive form.
// The tap loop of a tile row is gray_kernel's (vip_gray.hpp gray_row_taps), with the
// GrayAdaptiveDist index in place of the SAD.
// Both numerics profiles (FMA: explicit __builtin_fmaf; otherwise mul + add, the build
// has -ffp-contract=off) are instantiated here.
#include "vip_gray.hpp"

namespace vip {

constexpr int kGrayAdaP = 8, kGrayAdaWaves = 16;

// LDS words of the separable box sums' vertical pass: one u16 per tile row and plane column
template <int R>
constexpr int gray_adaptive_vsum_words() {
    using G = Geom<R, kGrayAdaP, 16>;
    return kGrayAdaWaves * G::RPW * (G::GROUPS * 4) / 2;
}
template <int R>
constexpr int gray_adaptive_lds_bytes() {
    using G = Geom<R, kGrayAdaP, 16>;
    return 4 * (kGrayAdaEntries * kGrayCopies + (kGrayAdaWaves * G::RPW + 2 * R) * G::S + gray_adaptive_vsum_words<R>());
}
// Do the LUT, the plane and the vertical sums fit the CU's LDS? With 16-bit column sums they
// do at every radius the kernel is built for (147,680 bytes at R = 15), so there is no
// per-thread square-sum form.
template <int R>
constexpr bool gray_adaptive_vbox() {
    return (2 * R + 1) * 255 < 65536 && gray_adaptive_lds_bytes<R>() <= kLdsBudget;
}
static_assert(gray_adaptive_vbox<1>() && gray_adaptive_vbox<kMaxRadius>(), "separable box sums at every radius built");

template <int R, bool FMA>
__global__ __launch_bounds__(kGrayAdaWaves * 64) void gray_adaptive_kernel(const StencilArgs a) {
    constexpr int P = kGrayAdaP, WAVES = kGrayAdaWaves, NT = WAVES * 64;
    using G = Geom<R, P, 16>;
    constexpr int TH = WAVES * G::RPW;
    constexpr int ROWS = TH + 2 * R;
    constexpr int K = 2 * R + 1;
    constexpr int VW = G::GROUPS * 4;  // plane words in use per row (TW + 2L)
    static_assert(gray_adaptive_vbox<R>(), "LUT + plane + vertical sums do not fit LDS");
    static_assert(TH % 4 == 0 && VW % 8 == 0, "vertical-sum runs of 4 rows; 16-byte aligned u16 rows");
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    uint32_t* const lut = lds;
    uint32_t* const plane = lds + kGrayAdaEntries * kGrayCopies;
    uint16_t* const vs = reinterpret_cast<uint16_t*>(plane + ROWS * G::S);  // TH x VW vertical K-row sums

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tx = lane & 15;
    const int ty = wave * G::RPW + (lane >> 4);
    const uint32_t lane4 = (uint32_t)(lane & (kGrayCopies - 1)) << 2;  // this lane's LUT copy
    const char* const lut_bytes = reinterpret_cast<const char*>(lut);

    // persistent: workgroup b filters tiles b, b + grid, ... (xcd_tile's placement)
    int tile = blockIdx.x;
    C1Prefetch<R, ROWS, NT, P, GrayGroup<0>> pf;
    LutStage<NT, kGrayAdaEntries, kGrayCopies> ls;
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
        // ---- pass 1a (whole workgroup): vertical K-row sums, 4 output rows per run ----
        // output row r <-> plane rows r .. r + 2R; every sum is an exact integer < 2^16
        for (int run = tid; run < VW * (TH / 4); run += NT) {
            const int c = run % VW, r0 = (run / VW) * 4;
            uint32_t x[4 + K - 1], o[4];
#pragma unroll
            for (int q = 0; q < 4 + K - 1; ++q) x[q] = plane[(r0 + q) * G::S + c];
            win_sum<4, K>(x, o);
#pragma unroll
            for (int j = 0; j < 4; ++j) vs[(r0 + j) * VW + c] = (uint16_t)o[j];
        }
        __syncthreads();
        if (ty0 + wave * G::RPW < a.out_rows) {  // wave-uniform: skip rows past the band
            GrayAdaptiveDist<P> dist;
            {
                // ---- pass 1b (per thread): K-column windows of the vertical sums ----
                constexpr int NCOLV = P + K - 1;
                constexpr int JB = G::L - R;  // first window column relative to tx * P
                constexpr int CB0 = JB / 4, CB1 = (G::L + P - 1 + R) / 4;
                uint32_t h[NCOLV], wsum[P];
                const uint16_t* const vrow = vs + ty * VW + tx * P;
#pragma unroll
                for (int c = CB0; c <= CB1; ++c) {
                    const uint2 g2 = *reinterpret_cast<const uint2*>(vrow + 4 * c);
                    const uint32_t g4[4] = {g2.x & 0xffffu, g2.x >> 16, g2.y & 0xffffu, g2.y >> 16};
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int j = 4 * c + q - JB;
                        if (j < 0 || j >= NCOLV) continue;
                        h[j] = g4[q];
                    }
                }
                win_sum<P, K>(h, wsum);
                const float kk = (float)(K * K);
                const float rkk = 1.f / kk;
                const uint4* c = reinterpret_cast<const uint4*>(plane + (ty + R) * G::S + tx * P + G::L);
#pragma unroll
                for (int q = 0; q < P / 4; ++q) {
                    const uint4 v = c[q];
                    dist.cf[4 * q + 0] = (float)v.x;
                    dist.cf[4 * q + 1] = (float)v.y;
                    dist.cf[4 * q + 2] = (float)v.z;
                    dist.cf[4 * q + 3] = (float)v.w;
                }
#pragma unroll
                for (int i = 0; i < P; ++i) {
                    // opaque to the optimiser (vip_adaptive.hip set_offsets): keeps n - c one v_sub_f32
                    __asm__("" : "+v"(dist.cf[i]));
                    dist.of[i] = dist.cf[i] - div_exact(wsum[i], kk, rkk);  // offset = centre - box mean
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
        __syncthreads();  // every wave is done reading this tile and its vertical sums
        pf.commit(plane);
        __syncthreads();
        tile = next;
    }
}

template <bool FMA>
static int launch_gray_adaptive_dispatch(int radius, const StencilArgs& a, hipStream_t stream) {
    return dispatch_radius(radius, [&](auto rc) {
        constexpr int R = decltype(rc)::value;
        return launch_c1_tiles<gray_adaptive_kernel<R, FMA>, gray_adaptive_lds_bytes<R>(), kGrayAdaWaves,
                               Geom<R, kGrayAdaP, 16>>(a, stream);
    });
}

int launch_gray_adaptive(int radius, bool fma, const StencilArgs& a, hipStream_t s) {
    return fma ? launch_gray_adaptive_dispatch<true>(radius, a, s) : launch_gray_adaptive_dispatch<false>(radius, a, s);
}

// ---------------------------------------------------------------- runtime radius
// 4 consecutive plane words as floats
struct GrayAdaRtWin {
    float c[4];
    __device__ __forceinline__ void load(const uint32_t* plane, int off) {
        const uint4 v = *reinterpret_cast<const uint4*>(plane + off);
        c[0] = (float)v.x; c[1] = (float)v.y; c[2] = (float)v.z; c[3] = (float)v.w;
    }
};

template <bool FMA>
__global__ __launch_bounds__(kRtWaves * 64) void gray_adaptive_rt_kernel(const RtArgs a) {
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

    // colour LUT: word d * 32 + c = color[d], d < 512
    for (int q = tid; q < kGrayAdaEntries * kGrayCopies / 4; q += NT) {
        const uint32_t v = __float_as_uint(a.color[q >> 3]);
        *reinterpret_cast<uint4*>(lut + 4 * q) = make_uint4(v, v, v, v);
    }
    // tile plane; columns [TW + 2L, S) and the pad are zeroed: the last tap block of a row
    // reads up to 4 words past its apron (weight 0), and a zero word's index against any
    // centre, int(|0 - 2c + mean|) <= 510, is still inside the table
    {
        const int gpr = S / 4, valid = (kRtTW + 2 * L) / 4;
        for (int q = tid; q < rows * gpr; q += NT) {
            const int r = q / gpr, gc = q - r * gpr;
            uint4 w = make_uint4(0u, 0u, 0u, 0u);
            if (gc < valid) {
                const int sy = clampi(ty0 + a.src_row0 - R + r, a.row_lo, a.row_hi - 1);
                GrayGroup<0> grp;
                grp.load(a.src, a.src_pitch, a.src, a.src_pitch, sy, tx0 - L + 4 * gc, a.width, a.aligned);
                w = grp.words();
            }
            *reinterpret_cast<uint4*>(plane + r * S + 4 * gc) = w;
        }
        if (L < 4 && tid < 2) *reinterpret_cast<uint4*>(plane + rows * S + 4 * tid) = make_uint4(0u, 0u, 0u, 0u);
    }
    __syncthreads();
    if (ty0 + wave * 4 >= a.out_rows) return;  // wave-uniform; no barrier follows

    const int xc = L + tx * P;  // plane column of the thread's output 0
    const uint32_t lanec = (uint32_t)(lane & (kGrayCopies - 1)) << 2;
    const char* const lut_bytes = reinterpret_cast<const char*>(lut);

    float cf[P], of[P];
    {
        // exact integer k x k sums per output: sliding row sums added into totals row by row
        const int K = 2 * R + 1;
        uint32_t tot[P];
#pragma unroll
        for (int i = 0; i < P; ++i) tot[i] = 0u;
        for (int r = 0; r < K; ++r) {
            const uint32_t* base = plane + (ty + r) * S + xc - R;
            uint32_t sum = 0u;
            for (int c = 0; c < K; ++c) sum += base[c];
#pragma unroll
            for (int i = 0; i < P; ++i) {
                if (i > 0) sum = sum + base[K - 1 + i] - base[i - 1];
                tot[i] += sum;
            }
        }
        // offset = centre - sum / (ksize * ksize), the IEEE quotient (radius 0: mean = c, o = 0)
        const float kk = (float)(K * K);
        const uint4 v = *reinterpret_cast<const uint4*>(plane + (ty + R) * S + xc);
        cf[0] = (float)v.x; cf[1] = (float)v.y; cf[2] = (float)v.z; cf[3] = (float)v.w;
#pragma unroll
        for (int i = 0; i < P; ++i) {
            __asm__("" : "+v"(cf[i]));  // keep (n - c) a float subtract (see gray_adaptive_kernel)
            of[i] = cf[i] - (float)tot[i] / kk;
        }
    }

    float s[P], sk[P];
#pragma unroll
    for (int i = 0; i < P; ++i) s[i] = sk[i] = 0.f;

    // 4 taps x 4 outputs: tap t of the block pairs output i with word t + i of cur|nxt
    auto block = [&](const GrayAdaRtWin& cur, const GrayAdaRtWin& nxt, const kconst float* wsb) {
        const float wsv[4] = {wsb[0], wsb[1], wsb[2], wsb[3]};  // uniform: one scalar load
        float wc[4][P];
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int i = 0; i < P; ++i) {
                const int j = t + i;
                const float n = j < 4 ? cur.c[j & 3] : nxt.c[j & 3];
                const uint32_t d = (uint32_t)__builtin_fabsf((n - cf[i]) - of[i]);
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
        GrayAdaRtWin A, B;
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

template <bool FMA>
static int launch_gray_adaptive_rt_f(RtArgs a, hipStream_t stream) {
    if (const int rc = rt_prepare(a)) return rc;
    const long long lds = 4LL * (rt_plane_words(a.R, a.L, a.S) + kGrayAdaEntries * kGrayCopies);
    return launch_rt_tiles<gray_adaptive_rt_kernel<FMA>>(a, lds, stream);
}

int launch_gray_adaptive_rt(const RtArgs& a, bool fma, hipStream_t s) {
    return fma ? launch_gray_adaptive_rt_f<true>(a, s) : launch_gray_adaptive_rt_f<false>(a, s);
}

}  // namespace vip
