// Bilateral and joint-bilateral filter kernels for gfx950 (MI355X).
//
// Behaviour follows src/bilateral_filter_impl.cu:7-202 of the reference
// (yuyuyu-bot/various_image_processings): per output pixel and per tap in
// row-major order, w = ws[ky,kx] * wc[|db|+|dg|+|dr|], sum_c += p_c * w,
// sumk += w, dst_c = u8(sum_c / sumk + 0.5f), replicate border. Taps outside
// the disc carry an exact zero weight in the reference and are skipped here,
// which leaves every sum bit-identical (x + 0*p == x).
//
// MI355X design: the kernel is FP32-VALU bound, not HBM bound,
// so everything is arranged to minimise VALU instructions per (output, tap):
//   v_sad_u8 (colour L1 distance of packed RGBX) -> v_lshl_or (LUT address)
//   -> ds_read_b32 (32-copy LUT, bank-conflict free) -> v_mul (spatial weight
//   from an SGPR) -> 3 x v_fma + v_add.
// Neighbour pixels are read once per thread-row with ds_read_b128 and shared by
// the thread's 8 horizontally adjacent outputs.
#include "vip_launch.hpp"
#include "vip_stencil.hpp"

namespace vip {

#ifdef VIP_STAMPS
// diagnostic build only: [block][wave][tile][3] shader-clock stamps
__device__ unsigned long long vip_stamps[256 * 16 * 8 * 3];
__device__ __forceinline__ void vip_stamp(int blk, int wave, int t, int k) {
    if ((threadIdx.x & 63) == 0 && t < 8 && blk < 256)
        vip_stamps[((blk * 16 + wave) * 8 + t) * 3 + k] = __builtin_amdgcn_s_memtime();
}
#define VIP_STAMP(t, k) vip_stamp(blockIdx.x, wave, t, k)
// [block][entry shader clock, entry 100 MHz real time, exit clock, exit real time]
__device__ unsigned long long vip_rt[256 * 4];
__device__ __forceinline__ void vip_rt_stamp(int k) {
    if (threadIdx.x == 0 && blockIdx.x < 256) {
        vip_rt[blockIdx.x * 4 + 2 * k] = __builtin_amdgcn_s_memtime();
        vip_rt[blockIdx.x * 4 + 2 * k + 1] = __builtin_amdgcn_s_memrealtime();
    }
}
#define VIP_RT_STAMP(k) vip_rt_stamp(k)
#else
#define VIP_STAMP(t, k)
#define VIP_RT_STAMP(k)
#endif

constexpr int kBilUnrollMaxR = 15;  // straight-line tile rows (for_each_row) up to this radius: all
constexpr bool kBilRcp = true;      // epilogue: one exact reciprocal per output instead of 3 IEEE divides
// NE: colour-LUT entries held in LDS. 768 (every L1 distance), or the folded tables' 32.
// FOLD (with SAT, NE = 32; the handle's LUT is exactly zero from entry 31 on -- small
// sigma_color: the texture filter's JBF has sigma_color sqrt(3), nonzero up to d = 24):
// one table per distinct squared tap distance r^2, holding
// the full weight RN(ws(r^2) * wc[d]) -- the same float product the unfolded taps
// form, so bit-identical -- addressed by the tap's compile-time table offset (the
// ds_read immediate) behind the saturating address (SatLut, vip_stencil.hpp): per tap
// v_sad_u8, v_mad_legacy_u16, 3 v_fma, v_add and no spatial v_mul, bank-conflict free.
// (Round 2 measured the folded tables behind a v_min clamp + v_lshl_or: 7 VALU, slower.)
template <int R>
struct FoldRank {  // table index of tap (|ky|, |kx|)
    int t[(R + 1) * (R + 1)];
    constexpr FoldRank() : t() {
        for (int y = 0; y <= R; ++y)
            for (int x = 0; x <= R; ++x) t[y * (R + 1) + x] = disc_r2_rank(R, x * x + y * y);
    }
};
// Largest |i - j| of a thread's outputs i, j whose centre-row weight is formed once and used by
// both (row_taps SHARE): 18 of the 28 pairs of 8 outputs, all 6 of 4 outputs, at most 6 weights
// held at once. At this distance the 4K kernels need no more registers than without sharing
// (VGPRs / spilled: C2's r = 7 108 / 0 as before, C5's r = 15 128 / 5 -> 4, the texture JBF's
// folded r = 4 128 / 1 -> 127 / 0). All 28 pairs (16 held at once) measured faster still at C2
// and the JBF but take 6 more VGPRs at C2 and spill in the kernels at the
// 128-VGPR limit (joint r = 7: 15 -> 20 spilled VGPRs, plain r = 15: 5 -> 11, no gain at C5).
constexpr int kPairShareDist = 3;
// The kernel body; MULTI: a multi-frame launch (bilateral_frames_kernel), whose tiles run
// from one frame into the next (StencilArgs::nframes). The one-frame kernel compiles with
// MULTI = false, to exactly the code it had before multi-frame launches existed.
template <int R, int WAVES, bool JOINT, bool FMA, int COPIES, int P, int NE, bool FOLD, int TPR, bool SAT, bool MULTI>
__device__ __forceinline__ void bilateral_body(const StencilArgs& a) {
    using G = Geom<R, P, TPR>;
    constexpr int NT = WAVES * 64;
    constexpr int TH = WAVES * G::RPW;
    constexpr bool ROW_UNROLL = R <= kBilUnrollMaxR;  // straight-line rows (for_each_row)
    constexpr int ROWS = TH + 2 * R;
    constexpr int PLANE = ROWS * G::S;
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    uint32_t* const lut = lds;
    constexpr int NTAB = FOLD ? disc_r2_count(R) : 1;
    static_assert(SAT == FOLD, "the saturating address serves the folded tables only");
    static_assert(!FOLD || (NE == 32 && COPIES == sat_fold_copies<R>()), "folded tables: saturating address");
    // SAT: one table per r^2 (d <= DZ) from byte SL::T, planes at SL::PL
    using SL = SatLut<R, 4 * (JOINT ? 2 : 1) * PLANE, disc_r2_count(R), kSatFoldDz, COPIES>;
    uint32_t* const gplane = SAT ? lds + SL::PL / 4 : lds + NTAB * NE * COPIES;
    uint32_t* const splane = JOINT ? gplane + PLANE : gplane;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tx = lane % TPR;
    const int ty = wave * G::RPW + lane / TPR;
    const uint32_t lane4 = (uint32_t)(lane & (COPIES - 1)) << 2;  // this lane's LUT copy
    const uint32_t sbias = (uint32_t)SL::B0 + lane4;                // SAT: register bias of the address
    const char* const lut_bytes = reinterpret_cast<const char*>(lut);
    // The centre tap's weight (kx = ky = 0, d = 0 for every output), once per thread: the
    // float product the tap formed, ws[0][0] * wc[0], or the folded table's entry (r^2 = 0, d = 0)
    // (wave-uniform: kept in a scalar register, the taps' v_fma take it as their one scalar operand)
    const float w0 = __uint_as_float(__builtin_amdgcn_readfirstlane(
        __float_as_uint(FOLD ? a.fold[disc_r2_rank(R, 0) * kFoldEntries] : a.color[0] * a.ws[0])));

    VIP_RT_STAMP(0);
    // persistent: workgroup b filters items b, b + grid, b + 2 grid, ... (item_tile: the
    // tiles; in a multi-frame launch the last round's tiles in pieces, plan_tail)
    int tile = blockIdx.x;
    const int items = launch_items<MULTI>(a);
    TilePrefetch<R, ROWS, NT, P, TPR> pg, ps;
    // once per workgroup; its reads go out first
    std::conditional_t<SAT, SatStage<NT, SL>, LutStage<NT, NTAB * NE, COPIES>> ls;
    ls.load(FOLD ? a.fold : a.color);
    // multi-frame launches (plain filter only: guide == src): frame f's tiles follow
    // frame f - 1's, so a workgroup's next tile may be the next frame's
    {
        const FrameTile ft = frame_tile<MULTI>(a, item_tile<MULTI>(a, tile));
        const int tx0 = (ft.t % a.tiles_x) * G::TW, ty0 = (ft.t / a.tiles_x) * TH;
        pg.issue(JOINT ? a.guide : frame_src<MULTI>(a.guide, ft.f), a.guide_pitch, a, tx0, ty0);
        if constexpr (JOINT) ps.issue(a.src, a.src_pitch, a, tx0, ty0);
    }
    ls.store(SAT ? lds + SL::T / 4 : lut);
    pg.commit(gplane);
    if constexpr (JOINT) ps.commit(splane);
    __syncthreads();

    for ([[maybe_unused]] int it = 0;; ++it) {
        VIP_STAMP(it, 0);
        const FrameTile ft = frame_tile<MULTI>(a, item_tile<MULTI>(a, tile));
        const int tx0 = (ft.t % a.tiles_x) * G::TW, ty0 = (ft.t / a.tiles_x) * TH;
        const int next = tile + (int)gridDim.x;
        if (next < items) {  // next tile's HBM reads fly under this tile's taps
            const FrameTile fn = frame_tile<MULTI>(a, item_tile<MULTI>(a, next));
            const int nx0 = (fn.t % a.tiles_x) * G::TW, ny0 = (fn.t / a.tiles_x) * TH;
            pg.issue(JOINT ? a.guide : frame_src<MULTI>(a.guide, fn.f), a.guide_pitch, a, nx0, ny0);
            if constexpr (JOINT) ps.issue(a.src, a.src_pitch, a, nx0, ny0);
        }
        // wave-uniform: skip rows past the frame, and other pieces' rows of a split tile
        if (ty0 + wave * G::RPW < a.out_rows && item_wave<MULTI, WAVES>(a, tile, wave)) {
            uint32_t ctr[P];  // centre pixels of the guide (== src for the plain filter)
            {
                const uint4* c = reinterpret_cast<const uint4*>(gplane + (ty + R) * G::S + tx * P + G::L);
#pragma unroll
                for (int q = 0; q < P / 4; ++q) {
                    const uint4 v = c[q];
                    ctr[4 * q + 0] = v.x; ctr[4 * q + 1] = v.y; ctr[4 * q + 2] = v.z; ctr[4 * q + 3] = v.w;
                }
            }
            f2 a01[P], a2k[P];  // {sum_b, sum_g}, {sum_r, sumk}
#pragma unroll
            for (int i = 0; i < P; ++i) a01[i] = a2k[i] = f2{0.f, 0.f};

            for_each_row<R, ROW_UNROLL>([&](const int ky, auto hwc) {
                    constexpr int HW = decltype(hwc)::value;
                    const int aky = ky < 0 ? -ky : ky;
                    set_progress_priority((ky + R) * 4 / (2 * R + 1));
                    const int row_off = (ty + R + ky) * G::S + tx * P;
                    const float* const ws = a.ws + aky * kWsStride;
                    constexpr int C0 = (G::L - HW) / 4, C1 = (G::L + P - 1 + HW) / 4;
                    constexpr int NC = C1 - C0 + 1;
                    float wsv[HW + 1];
#pragma unroll
                    for (int k = 0; k <= HW; ++k) wsv[k] = ws[k];
                    // colour weight address: v_sad_u8 (|db|+|dg|+|dr|) -> word d*COPIES + lane copy
                    auto widx = [&](uint32_t g, f2, f2, int i, int kx) {
                        uint32_t d = __builtin_amdgcn_sad_u8(g, ctr[i], 0u);
                        if constexpr (FOLD) {  // min(d*S + bias, 65535) + table offset (immediate)
                            constexpr FoldRank<R> rank;
                            return sat_addr(d, SL::S, sbias) + (uint32_t)(SL::T - SL::B0) +
                                   4u * COPIES * rank.t[aky * (R + 1) + (kx < 0 ? -kx : kx)];
                        }
                        return (d << (COPIES == 32 ? 7 : 6)) | lane4;
                    };
                    // the outputs' own row shares each in-thread pair's weight and takes w0 at
                    // the centre tap (row_taps SHARE); ky is a constant in the unrolled rows
                    if (ky == 0)
                        row_taps<HW, G::L, C0, NC, FMA, P, JOINT, decltype(widx)&, FOLD, kPipeDepth, SAT,
                                 kPairShareDist>(
                            gplane, splane, row_off, wsv, lut_bytes, widx, a01, a2k, w0);
                    else
                        row_taps<HW, G::L, C0, NC, FMA, P, JOINT, decltype(widx)&, FOLD, kPipeDepth, SAT>(
                            gplane, splane, row_off, wsv, lut_bytes, widx, a01, a2k);
                    if constexpr (ROW_UNROLL) fence_accumulators(a01, a2k);
            });

            uint32_t o[P];
            finish_outputs<P, kBilRcp>(a01, a2k, o);
            store_px_to(a, JOINT ? a.dst : frame_dst<MULTI>(a, tile), ty0 + ty, tx0 + tx * P, o);
        }
        VIP_STAMP(it, 1);
        if (next >= items) {
            VIP_RT_STAMP(1);
            break;
        }
        __syncthreads();  // every wave is done reading this tile
        pg.commit(gplane);
        if constexpr (JOINT) ps.commit(splane);
        __syncthreads();
        VIP_STAMP(it, 2);
        tile = next;
    }
}

template <int R, int WAVES, bool JOINT, bool FMA, int COPIES, int P, int NE = 768, bool FOLD = false, int TPR = 16,
          bool SAT = false>
__global__ __launch_bounds__(WAVES * 64) void bilateral_kernel(const StencilArgs a) {
    bilateral_body<R, WAVES, JOINT, FMA, COPIES, P, NE, FOLD, TPR, SAT, false>(a);
}
// multi-frame launches (vip_bilateral_run_rows_batch; plain filter, radius <= kBatchMaxRadius)
template <int R, int WAVES, bool JOINT, bool FMA, int COPIES, int P, int NE = 768, bool FOLD = false, int TPR = 16,
          bool SAT = false>
__global__ __launch_bounds__(WAVES * 64) void bilateral_frames_kernel(const StencilArgs a) {
    bilateral_body<R, WAVES, JOINT, FMA, COPIES, P, NE, FOLD, TPR, SAT, true>(a);
}

// The joint kernel holds two tile planes; when the full 32-copy LUT leaves room for
// fewer than 16 waves, a 16-copy LUT (lanes l and l+16 of a half-wave share a copy:
// at most 2-way bank conflicts) is used if it buys more waves.
constexpr bool kJbfLut16 = true;
// Outputs per thread: 8 for the plain filter. The joint filter's second plane and
// prefetch registers push 8 outputs past 128 VGPRs as the radius grows (spilled
// VGPRs: 0 up to R = 3, 1 at R = 4, 14 at R = 7, 36 at R = 8, 69+ beyond); 8 outputs
// still win up to R = 7 (measured: r=4 84 -> 79 us, r=7 214 -> 206 us), 4 above
// (round 6, texture JBF at 4K, profiles/r06_jbf_p8_big_r_ab.txt: R = 8 239.7-240.0 us with
// 4 outputs on 16 waves against 266.4-266.6 with 8 on 12 waves).
constexpr int kJbfP8MaxR = 7;
constexpr int kBilP = 8;
template <int R, int PLANES>
constexpr int outputs_per_thread() { return PLANES == 2 ? (R <= kJbfP8MaxR ? 8 : 4) : kBilP; }
template <int R, int PLANES>
constexpr int lut_copies() {
    constexpr int P = outputs_per_thread<R, PLANES>();
    if (!kJbfLut16 || PLANES == 1) return 32;
    return pick_waves<R, PLANES, 16, 768 * 16, P>() > pick_waves<R, PLANES, 16, 768 * 32, P>() ? 16 : 32;
}

// Small frames (plain filter, R <= kBilSmallMaxR): a frame with fewer 128 x 64
// tiles than CUs leaves CUs idle (C1's 512 x 512 lenna: 32 tiles on 256 CUs; a 270-row
// slab of the 4K frame at 8 GPUs: 150). Two ways to spread it: fewer waves per workgroup
// (8 or 4: 128 x 32 / 128 x 16 tiles, more CUs busy, fewer waves per SIMD), and the
// "wide" tiling -- one 256-pixel row per wave, 4 outputs per thread -- which halves the
// serial tap work of a thread, so a launch whose tiles fit in one round ends sooner
// (every thread of a 16-wave tile runs its 8 outputs x 149 taps back to back: ~47 us
// at r = 7, whatever the frame size). Chosen per launch by a per-CU time model,
// rounds * waves * cost(waves) * work(P): cost = 1, 1.25, 1.8 at 4, 2, 1 waves per SIMD,
// work = 1 for 8 outputs per thread, kWideWork for 4 (half the taps plus the extra byte
// conversions and apron rows). vip_bilateral_set_waves / VIP_BIL_WAVES and
// vip_bilateral_set_wide / VIP_BIL_WIDE force either.
constexpr int kBilSmallMaxR = 8;
constexpr float kWideWork = 0.55f;
struct Tiling {
    int waves;
    bool wide;
};
// With F frames in flight (distinct streams among the device's recent launches,
// vip_capi.hip frames_in_flight) the frames share the chip, so a frame's rounds are counted
// on cus / F CUs: a small frame then takes the tiling that fills its share, not the one
// that ends soonest alone (C1 with 4 streams: 16-wave 256-px tiles, 61.8k against 27.3k
// Mpx/s for the one-frame choice, profiles/r03 small-frame tables in DESIGN.md section 4).
inline Tiling small_frame_tiling(int width, int out_rows, int inflight = 1, int nframes = 1) {
    const int forced = bilateral_forced_waves();
    const int fwide = bilateral_forced_wide();  // 0 auto, 1 narrow, 2 wide
    const int share = device_cus() / (inflight > 1 ? inflight : 1);  // CUs per launch
    const int cus = share > 0 ? share : 1;
    const int cand[3] = {16, 8, 4};
    const float cost[3] = {1.0f, 1.25f, 1.8f};
    Tiling best{16, false};
    float best_t = 0.f;
    bool first = true;
    for (int wide = 0; wide < 2; ++wide) {
        if ((fwide == 1 && wide) || (fwide == 2 && !wide) || (fwide == 0 && forced && wide)) continue;
        const int tw = wide ? 256 : 128, rpw = wide ? 1 : 4;
        const long long tiles_x = (width + tw - 1) / tw;
        for (int i = 0; i < 3; ++i) {
            if (forced && cand[i] != forced) continue;
            const int th = cand[i] * rpw;
            const long long tiles = tiles_x * ((out_rows + th - 1) / th) * (nframes > 1 ? nframes : 1);
            const float t = (float)((tiles + cus - 1) / cus) * cand[i] * cost[i] * (wide ? kWideWork : 1.f);
            if (first || t < best_t) best = Tiling{cand[i], wide != 0}, best_t = t, first = false;
        }
    }
    return best;
}

// The launch with its wave count chosen. FOLD: the joint filter's folded tables behind the
// saturating address (SatLut), 32 entries; otherwise the 768-entry colour LUT. WIDE: 256-pixel
// tiles (plain filter only).
template <int R, bool JOINT, bool FMA, bool FOLD, int WAVES, bool WIDE = false>
static int launch_bilateral_w(const StencilArgs& a, hipStream_t stream);

// LDS of a folded launch (the saturating-address tables and the planes)
template <int R, int WAVES, int PLANES, int P>
constexpr int sat_lds_bytes() {
    return SatLut<R, 4 * PLANES * (WAVES * Geom<R, P>::RPW + 2 * R) * Geom<R, P>::S, disc_r2_count(R), kSatFoldDz,
                  sat_fold_copies<R>()>::BYTES;
}
template <int R, int PLANES, int P>
constexpr int pick_waves_sat() {
    if (sat_lds_bytes<R, 16, PLANES, P>() <= kLdsBudget) return 16;
    if (sat_lds_bytes<R, 12, PLANES, P>() <= kLdsBudget) return 12;
    if (sat_lds_bytes<R, 8, PLANES, P>() <= kLdsBudget) return 8;
    return sat_lds_bytes<R, 4, PLANES, P>() <= kLdsBudget ? 4 : 0;
}

template <int R, bool JOINT, bool FMA, bool FOLD>
static int launch_bilateral_lut(const StencilArgs& a, hipStream_t stream) {
    constexpr int PLANES = JOINT ? 2 : 1;
    constexpr int P = outputs_per_thread<R, PLANES>();
    constexpr int WAVES = FOLD ? pick_waves_sat<R, PLANES, P>()
                               : pick_waves<R, PLANES, 16, 768 * lut_copies<R, PLANES>(), P>();
    static_assert(WAVES > 0, "tile does not fit LDS");
    if constexpr (!JOINT && WAVES == 16 && R <= kBilSmallMaxR) {
        const Tiling t = small_frame_tiling(a.width, a.out_rows, a.inflight, a.nframes);
        if (t.wide) {
            if (t.waves == 16) return launch_bilateral_w<R, JOINT, FMA, FOLD, 16, true>(a, stream);
            if (t.waves == 8) return launch_bilateral_w<R, JOINT, FMA, FOLD, 8, true>(a, stream);
            return launch_bilateral_w<R, JOINT, FMA, FOLD, 4, true>(a, stream);
        }
        if (t.waves == 8) return launch_bilateral_w<R, JOINT, FMA, FOLD, 8>(a, stream);
        if (t.waves == 4) return launch_bilateral_w<R, JOINT, FMA, FOLD, 4>(a, stream);
    }
    return launch_bilateral_w<R, JOINT, FMA, FOLD, WAVES>(a, stream);
}

template <int R, bool JOINT, bool FMA, bool FOLD, int WAVES, bool WIDE>
static int launch_bilateral_w(const StencilArgs& a, hipStream_t stream) {
    static_assert(!FOLD || JOINT, "folded tables: the joint filter");
    static_assert(!WIDE || !JOINT, "wide tiles: the plain filter");
    constexpr int PLANES = JOINT ? 2 : 1;
    constexpr int P = WIDE ? 4 : outputs_per_thread<R, PLANES>();
    constexpr int TPR = WIDE ? 64 : 16;  // threads per tile row
    using G = Geom<R, P, TPR>;
    constexpr int NE = FOLD ? kFoldEntries : 768;
    constexpr int COPIES = FOLD ? sat_fold_copies<R>() : lut_copies<R, PLANES>();
    constexpr int TH = WAVES * G::RPW;
    constexpr int LDS = FOLD ? sat_lds_bytes<R, WAVES, PLANES, P>() : lds_bytes<R, WAVES, PLANES, NE * COPIES, P, TPR>();
    static_assert(LDS <= kLdsBudget, "tile does not fit LDS");
    constexpr bool SAT = FOLD;  // the kernel's saturating address (absolute LDS addresses)
    constexpr auto kern = bilateral_kernel<R, WAVES, JOINT, FMA, COPIES, P, NE, FOLD, TPR, SAT>;
    if constexpr (!JOINT && R <= kBatchMaxRadius) {
        constexpr auto frames_kern = bilateral_frames_kernel<R, WAVES, JOINT, FMA, COPIES, P, NE, FOLD, TPR, SAT>;
        // the last round in pieces for one frame in flight only: with two streams the other
        // stream's launch already fills the CUs a whole-tile last round leaves idle, and the
        // pieces' fewer waves per CU cost more CU time (C2 slab at 8 GPUs, 6 frames per launch,
        // 8 CUs free: one stream 0.0256-0.0258 -> 0.0250 ms per frame, two streams 0.0222-0.0225
        // -> 0.0231-0.0233; profiles/r05_slab_batch_ab{,2}.txt)
        return launch_persistent<kern, frames_kern, LDS, WAVES, G::TW, TH, SAT>(a, a.inflight <= 1, stream);
    } else {
        // no multi-frame form (the batch entry point loops frames); the joint filter is one frame
        if (!JOINT && a.nframes > 1) return VIP_ERR_INVALID_ARGUMENT;
        return launch_persistent<kern, nullptr, LDS, WAVES, G::TW, TH, SAT>(a, false, stream);
    }
}

template <int R, bool JOINT, bool FMA>
static int launch_bilateral_r(const StencilArgs& a, hipStream_t stream) {
    if constexpr (JOINT && R <= kSatMaxR)  // saturating-address folded tables (SatLut)
        if (a.fold && a.lut_nonzero <= SatLut<R, 0, disc_r2_count(R), kSatFoldDz, sat_fold_copies<R>()>::DZ)
            return launch_bilateral_lut<R, JOINT, FMA, true>(a, stream);
    return launch_bilateral_lut<R, JOINT, FMA, false>(a, stream);
}

template <bool JOINT, bool FMA>
static int launch_bilateral_dispatch(int radius, const StencilArgs& a, hipStream_t stream) {
    switch (radius) {
#define VIP_CASE(RR) \
    case RR: return launch_bilateral_r<RR, JOINT, FMA>(a, stream);
#ifdef VIP_ONLY_R7
        VIP_CASE(4) VIP_CASE(7) VIP_CASE(15)
#else
        VIP_CASE(1) VIP_CASE(2) VIP_CASE(3) VIP_CASE(4) VIP_CASE(5) VIP_CASE(6) VIP_CASE(7) VIP_CASE(8)
        VIP_CASE(9) VIP_CASE(10) VIP_CASE(11) VIP_CASE(12) VIP_CASE(13) VIP_CASE(14) VIP_CASE(15)
#endif
#undef VIP_CASE
        default: return VIP_ERR_UNSUPPORTED_KSIZE;
    }
}

// One translation unit per (JOINT, FMA) variant so the 15 radii compile in parallel.
#if defined(VIP_BIL_JOINT) && defined(VIP_BIL_FMA)
int launch_bilateral_joint_fma(int radius, const StencilArgs& a, hipStream_t s) {
    return launch_bilateral_dispatch<true, true>(radius, a, s);
}
#elif defined(VIP_BIL_JOINT)
int launch_bilateral_joint_mul(int radius, const StencilArgs& a, hipStream_t s) {
    return launch_bilateral_dispatch<true, false>(radius, a, s);
}
#elif defined(VIP_BIL_FMA)
int launch_bilateral_plain_fma(int radius, const StencilArgs& a, hipStream_t s) {
    return launch_bilateral_dispatch<false, true>(radius, a, s);
}
#ifdef VIP_STAMPS
}  // namespace vip
extern "C" int vip_debug_read_stamps(void* host, size_t bytes) {
    return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(vip::vip_stamps), bytes, 0, hipMemcpyDeviceToHost);
}
extern "C" int vip_debug_read_rt(void* host, size_t bytes) {
    return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(vip::vip_rt), bytes, 0, hipMemcpyDeviceToHost);
}
namespace vip {
#endif
#else
int launch_bilateral_plain_mul(int radius, const StencilArgs& a, hipStream_t s) {
    return launch_bilateral_dispatch<false, false>(radius, a, s);
}
#endif

}  // namespace vip
