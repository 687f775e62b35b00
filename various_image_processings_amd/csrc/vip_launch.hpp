// Host-to-kernel interface of the stencil and texture kernels: the argument structs the
// C ABI (vip_capi.hip) fills, the constants it reads, the host-side launch helpers, and
// one declaration of every launcher that crosses translation units. No device code: the
// tile and tap machinery is vip_stencil.hpp.
#pragma once

#include <atomic>
#include <type_traits>
#include <utility>

#include <hip/hip_ext.h>

#include "vip_common.hpp"

namespace vip {

constexpr int kMaxRadius = 15;            // ksize <= 31 (BASELINE C5 uses ksize 31)
constexpr int kWsStride = kMaxRadius + 1; // spatial weights stored as ws[|ky|][|kx|]
constexpr int kP = 8;                     // outputs per thread
constexpr int kTW = 16 * kP;              // tile width in pixels
constexpr int kLdsBudget = 160 * 1024;
// joint kernel: folded tables behind a saturating address (SatLut) up to this radius. 7 and 8
// work with 16-copy tables (sat_fold_copies), bit-exact, but measured slower than the
// 768 x 16 LUT those radii keep: texture JBF R = 7 186.6 -> 207.8 us, R = 8 242.0 -> 274.7
// (profiles/r06_jbf_fold16_ab.txt)
constexpr int kSatMaxR = 6;
constexpr int kFoldEntries = 32;  // the handle's folded tables hold d < 32 (zeros past the colour LUT's end)

// Frames one launch of the plain bilateral / adaptive kernels may filter (the
// *_run_rows_batch entry points; a shard's B frames per RCCL group, vip_shard_run_batch).
constexpr int kMaxBatchFrames = 6;
// Radii whose plain / adaptive kernels have a multi-frame form (the small-slab radii; a
// batch of larger radii launches frame by frame)
constexpr int kBatchMaxRadius = 8;

struct StencilArgs {
    const uint8_t* src;
    const uint8_t* guide;  // == src for the plain filters
    uint8_t* dst;
    long long src_pitch, guide_pitch, dst_pitch;
    int width;
    int out_rows;          // output rows to produce
    int src_row0;          // source row of output row 0
    int row_lo, row_hi;    // neighbour rows clamp to [row_lo, row_hi)
    int tiles_x;
    int tiles_total;       // tiles_x * tiles_y (persistent workgroups stride over them)
    int aligned;           // src/guide base and pitch are 4-byte aligned -> dword tile loads
    int dst_aligned;       // dst base and pitch are 8-byte aligned -> qword stores
    const float* color;    // colour LUT in device memory
    int lut_nonzero;       // entries [lut_nonzero, end) of the colour LUT are exactly 0
    const float* fold;     // or null: [disc_r2_count(R)][kFoldEntries] = RN(ws(r^2) * colour[d])
    int inflight;          // host only: frames in flight on this device (the small-frame tiling's model)
    // Multi-frame launch: frame f < nframes reads fsrc[f] and writes fdst[f] (fsrc[0] == src,
    // fdst[0] == dst; same geometry and pitches); launch tile t is tile t - f * tiles_frame of
    // frame f, so the persistent workgroups run straight from one frame's tiles into the
    // next one's (one prologue, the next tile's loads under the current one's taps).
    int nframes;
    int tiles_frame;       // tiles per frame (set by the launcher)
    int free_cus;          // host only: persistent workgroups leave this many CUs to concurrent work
    // Last-round split (multi-frame kernels, plan_tail): launch tiles [tail_full, tiles_total)
    // run in the last round as 2^tail_shift pieces each, a piece being a run of the tile's
    // waves; tail_full == tiles_total and tail_shift == 0 when the rounds come out even.
    int tail_full, tail_shift;
    const uint8_t* fsrc[kMaxBatchFrames];
    uint8_t* fdst[kMaxBatchFrames];
    float ws[kWsStride * kWsStride];  // spatial LUT, |ky|-major, in the kernarg segment (scalar loads)
};

// Runtime-radius kernels (vip_stencil_rt.hip and the one-channel ones; their shared frame and
// its launch helpers rt_prepare / launch_rt_tiles: vip_rt.hpp): radius 0 and the radii above
// the templated set, up to the reference's largest (bilateral ksize 65).
constexpr int kRtMaxRadius = 32;

struct RtArgs {
    const uint8_t* src;
    const uint8_t* guide;  // == src for the plain filters
    uint8_t* dst;
    long long src_pitch, guide_pitch, dst_pitch;
    int width, out_rows, src_row0, row_lo, row_hi;  // as StencilArgs
    int aligned, dst_aligned;  // as StencilArgs, but dst_aligned: 4-byte aligned -> dword stores
    const float* color;    // colour LUT (768 or 1536 entries)
    const float* wsrow;    // [2R+1][wst]: ws(kx, ky) at [ky + R][kx + ra], 0 outside the disc
    const int* hw;         // [R+1]: disc half-width of row |ky|
    int R, wst, ra;
    int L, S, tiles_x;     // set by the launcher
};

// The launchers: vip_bilateral.hip (one translation unit per joint/fma pair), vip_adaptive.hip
// (one per arithmetic), vip_stencil_rt.hip, vip_gray.hip, vip_gray_adaptive.hip, then vip_texture.hip and vip_gray_texture.hip. The stencil launchers
// return VIP_ERR_UNSUPPORTED_KSIZE for a radius they have no kernel for.
int launch_bilateral_joint_fma(int radius, const StencilArgs& a, hipStream_t s);
int launch_bilateral_joint_mul(int radius, const StencilArgs& a, hipStream_t s);
int launch_bilateral_plain_fma(int radius, const StencilArgs& a, hipStream_t s);
int launch_bilateral_plain_mul(int radius, const StencilArgs& a, hipStream_t s);
int launch_adaptive_fma(int radius, const StencilArgs& a, hipStream_t s);
int launch_adaptive_mul(int radius, const StencilArgs& a, hipStream_t s);
int launch_stencil_rt(const RtArgs& a, bool joint, bool adaptive, bool fma, hipStream_t stream);
// vip_gray.hip: one-channel source and destination; guide_channels 0 (plain: the source is its
// own guide), 1 (gray guide) or 3 (interleaved 3-channel guide); radius 1..15 / runtime radius
int launch_gray(int radius, int guide_channels, bool fma, const StencilArgs& a, hipStream_t s);
int launch_gray_rt(const RtArgs& a, int guide_channels, bool fma, hipStream_t s);
// vip_gray_adaptive.hip: the one-channel adaptive filter; radius 1..15 / runtime radius
int launch_gray_adaptive(int radius, bool fma, const StencilArgs& a, hipStream_t s);
int launch_gray_adaptive_rt(const RtArgs& a, bool fma, hipStream_t s);
// vip_joint_f32.hip: f32 one-channel source and destination under an 8-bit guide (guide_channels
// 1 or 3); radius 1..15 / runtime radius 0..23. src and dst carry the float pointers, pitches in
// bytes; `aligned` is a set of the bits below and dst_aligned means base and pitch are 16-byte
// aligned (float4 stores), both set by the entry point (vip_joint_bilateral_run_rows_f32)
constexpr int kF32GuideWords = 1;  // guide base and pitch are 4-byte aligned -> dword guide loads
constexpr int kF32SrcVec = 2;      // source base and pitch are 16-byte aligned -> float4 loads
int launch_joint_f32(int radius, int guide_channels, bool fma, const StencilArgs& a, hipStream_t s);
int launch_joint_f32_rt(const RtArgs& a, int guide_channels, bool fma, hipStream_t s);
// vip_upsample.hip: joint bilateral upsampling of a low-resolution f32 field (src, with the
// low-resolution guide guide_lo beside it) under the full-resolution 8-bit guide; radius
// 0..kUpMaxRadius in low-resolution pixels, scale 2, 4 or 8, guide_channels 1 or 3. src and dst
// carry the float pointers, pitches in bytes; `aligned` is a set of kF32GuideWords and kF32SrcVec
// (the low-resolution pair) and kUpGuideWords, dst_aligned as launch_joint_f32's.
constexpr int kUpMaxRadius = 4;   // ksize <= 9
constexpr int kUpGuideWords = 4;  // full-resolution guide base and pitch are 4-byte aligned -> dword loads
struct UpsampleArgs {
    const uint8_t* src;
    const uint8_t* guide_lo;
    const uint8_t* guide;
    uint8_t* dst;
    long long src_pitch, guide_lo_pitch, guide_pitch, dst_pitch;
    int width, out_rows;          // the output frame (out_rows: its height)
    int low_width, low_height;    // ceil(width / scale), ceil(out_rows / scale)
    int tiles_x, tiles_total;     // set by the launcher
    int aligned, dst_aligned;
    const float* color;           // colour LUT in device memory (768 entries)
    const float* wsp;             // [n][n], n = scale * radius + scale / 2: the spatial weight of the offset
                                  // (2 ax + 1, 2 ay + 1) half pixels at [ay][ax]
};
int launch_upsample_f32(int radius, int scale, int guide_channels, bool fma, const UpsampleArgs& a, hipStream_t s);
// vip_upsample_f32c.hpp: launch_upsample_f32's filter on an interleaved field of channels = 2..4, every
// radius and scale. UpsampleArgs exactly as launch_upsample_f32 reads it: a cell of src and a pixel
// of dst are C floats. One translation unit per channel count (vip_upsample_f32c_c2.hip, _c3, _c4)
// instantiates the template.
template <int C>
int launch_upsample_f32c_channels(int radius, int scale, int guide_channels, bool fma, const UpsampleArgs& a,
                                  hipStream_t s);
// each unit compiles its own channel count only, also where it sees the template's definition
extern template int launch_upsample_f32c_channels<2>(int, int, int, bool, const UpsampleArgs&, hipStream_t);
extern template int launch_upsample_f32c_channels<3>(int, int, int, bool, const UpsampleArgs&, hipStream_t);
extern template int launch_upsample_f32c_channels<4>(int, int, int, bool, const UpsampleArgs&, hipStream_t);
inline int launch_upsample_f32c(int radius, int scale, int channels, int guide_channels, bool fma,
                                const UpsampleArgs& a, hipStream_t s) {
    switch (channels) {
        case 2: return launch_upsample_f32c_channels<2>(radius, scale, guide_channels, fma, a, s);
        case 3: return launch_upsample_f32c_channels<3>(radius, scale, guide_channels, fma, a, s);
        case 4: return launch_upsample_f32c_channels<4>(radius, scale, guide_channels, fma, a, s);
        default: return VIP_ERR_INVALID_ARGUMENT;
    }
}
// vip_joint_conf.hip: the confidence-weighted form of launch_joint_f32 (radius 0..15, no
// runtime-radius kernel). StencilArgs as launch_joint_f32 reads it (one whole frame), plus the
// confidence plane, the optional weight output and the value written where no weight was in reach;
// the struct is this kernel's alone, so every other kernel's arguments stay what they are.
struct ConfArgs : StencilArgs {
    const uint8_t* conf;   // f32 confidence, pitch in bytes
    uint8_t* weight;       // f32 sum of weights, or null
    long long conf_pitch, weight_pitch;
    float hole_value;
    int conf_vec;          // conf base and pitch are 16-byte aligned -> float4 loads
    int weight_aligned;    // weight base and pitch are 16-byte aligned -> float4 stores
};
int launch_joint_conf_f32(int radius, int guide_channels, bool fma, const ConfArgs& a, hipStream_t s);
// vip_joint_f32c.hip: launch_joint_f32's filter on an interleaved f32 source of channels = 2..4
// (radius 0..15 at C = 2, 0..7 at C = 3 and 4, VIP_ERR_UNSUPPORTED_KSIZE beyond; no runtime-radius
// kernel). StencilArgs exactly as launch_joint_f32 reads it: a pixel of src and dst is C floats.
int launch_joint_f32c(int radius, int channels, int guide_channels, bool fma, const StencilArgs& a, hipStream_t s);
// vip_bilateral_f32.hpp: the self-guided f32 bilateral filter (radius 0..15, no runtime-radius
// kernel). StencilArgs as launch_joint_f32 reads it, without a guide (guide == src, never read as
// one): src and dst carry the float pointers, `aligned` holds kF32SrcVec, dst_aligned means 16-byte
// aligned, and color points at the handle's range table: kBf32Pairs (L[i], D[i]) float pairs,
// i = 0..VIP_BILATERAL_F32_BINS. The struct is this kernel's alone.
constexpr int kBf32Pairs = VIP_BILATERAL_F32_BINS + 1;
struct BilateralF32Args : StencilArgs {
    float scale;  // (float)VIP_BILATERAL_F32_BINS / value_range
};
// vip_bilateral_f32.hpp is instantiated by one unit per arithmetic and radius group (part),
// vip_bilateral_f32_fma_p0.hip .. _mul_p3.hip: each defines one specialization of
// launch_bilateral_f32_part, for the radii kBf32PartLo[part]..kBf32PartHi[part].
constexpr int kBf32Parts = 4;
constexpr int kBf32PartLo[kBf32Parts] = {0, 12, 14, 15};
constexpr int kBf32PartHi[kBf32Parts] = {11, 13, 14, 15};
static_assert(kBf32PartHi[kBf32Parts - 1] == kMaxRadius, "the parts cover radius 0..kMaxRadius");
template <bool FMA, int PART>
int launch_bilateral_f32_part(int radius, const BilateralF32Args& a, hipStream_t s);
#define VIP_BF32_DECLARE_PART(FMA, PART) \
    template <>                          \
    int launch_bilateral_f32_part<FMA, PART>(int radius, const BilateralF32Args& a, hipStream_t s);
VIP_BF32_DECLARE_PART(true, 0) VIP_BF32_DECLARE_PART(true, 1) VIP_BF32_DECLARE_PART(true, 2) VIP_BF32_DECLARE_PART(true, 3)
VIP_BF32_DECLARE_PART(false, 0) VIP_BF32_DECLARE_PART(false, 1) VIP_BF32_DECLARE_PART(false, 2) VIP_BF32_DECLARE_PART(false, 3)
#undef VIP_BF32_DECLARE_PART
template <bool FMA>
inline int launch_bilateral_f32_fma(int radius, const BilateralF32Args& a, hipStream_t s) {
    if (radius < 0 || radius > kMaxRadius) return VIP_ERR_UNSUPPORTED_KSIZE;
    if (radius <= kBf32PartHi[0]) return launch_bilateral_f32_part<FMA, 0>(radius, a, s);
    if (radius <= kBf32PartHi[1]) return launch_bilateral_f32_part<FMA, 1>(radius, a, s);
    if (radius <= kBf32PartHi[2]) return launch_bilateral_f32_part<FMA, 2>(radius, a, s);
    return launch_bilateral_f32_part<FMA, 3>(radius, a, s);
}
inline int launch_bilateral_f32(int radius, bool fma, const BilateralF32Args& a, hipStream_t s) {
    return fma ? launch_bilateral_f32_fma<true>(radius, a, s) : launch_bilateral_f32_fma<false>(radius, a, s);
}
// vip_bilateral_f32c.hpp: launch_bilateral_f32's filter on an interleaved f32 image of channels = 2 or 3,
// the range weight from the L1 distance over the channels (radius 0..kBf32cMaxRadius,
// VIP_ERR_UNSUPPORTED_KSIZE beyond; no runtime-radius kernel). BilateralF32Args exactly as
// launch_bilateral_f32 reads it: a pixel of src and dst is C floats. One translation unit per channel
// count and arithmetic (vip_bilateral_f32c_c2_fma.hip .. _c3_mul.hip) instantiates the template.
constexpr int kBf32cMaxRadius = 7;
template <int C, bool FMA>
int launch_bilateral_f32c_unit(int radius, const BilateralF32Args& a, hipStream_t s);
// each unit compiles its own pair only, also where it sees the template's definition
extern template int launch_bilateral_f32c_unit<2, true>(int, const BilateralF32Args&, hipStream_t);
extern template int launch_bilateral_f32c_unit<2, false>(int, const BilateralF32Args&, hipStream_t);
extern template int launch_bilateral_f32c_unit<3, true>(int, const BilateralF32Args&, hipStream_t);
extern template int launch_bilateral_f32c_unit<3, false>(int, const BilateralF32Args&, hipStream_t);
inline int launch_bilateral_f32c(int radius, int channels, bool fma, const BilateralF32Args& a, hipStream_t s) {
    if (radius < 0 || radius > kBf32cMaxRadius) return VIP_ERR_UNSUPPORTED_KSIZE;
    switch (channels) {
        case 2: return fma ? launch_bilateral_f32c_unit<2, true>(radius, a, s) : launch_bilateral_f32c_unit<2, false>(radius, a, s);
        case 3: return fma ? launch_bilateral_f32c_unit<3, true>(radius, a, s) : launch_bilateral_f32c_unit<3, false>(radius, a, s);
        default: return VIP_ERR_INVALID_ARGUMENT;
    }
}
// vip_bilateral_f32j.hpp: launch_bilateral_f32's filter with the distance taken from a second f32
// one-channel image, the guide (radius 0..15, no runtime-radius kernel). BilateralF32Args as
// launch_bilateral_f32 reads it, with guide and guide_pitch the float guide's (guide == src is
// allowed and still read as a guide); `aligned` is a set of kF32SrcVec and kF32GuideVec. One unit
// per arithmetic and radius group, vip_bilateral_f32j_fma_p0.hip .. _mul_p3.hip, as above.
constexpr int kF32GuideVec = 8;  // float guide base and pitch are 16-byte aligned -> float4 loads
constexpr int kBf32jParts = 4;
constexpr int kBf32jPartLo[kBf32jParts] = {0, 12, 14, 15};
constexpr int kBf32jPartHi[kBf32jParts] = {11, 13, 14, 15};
static_assert(kBf32jPartHi[kBf32jParts - 1] == kMaxRadius, "the parts cover radius 0..kMaxRadius");
template <bool FMA, int PART>
int launch_bilateral_f32_joint_part(int radius, const BilateralF32Args& a, hipStream_t s);
// each unit compiles its own specialization only
template <> int launch_bilateral_f32_joint_part<true, 0>(int radius, const BilateralF32Args& a, hipStream_t s);
template <> int launch_bilateral_f32_joint_part<true, 1>(int radius, const BilateralF32Args& a, hipStream_t s);
template <> int launch_bilateral_f32_joint_part<true, 2>(int radius, const BilateralF32Args& a, hipStream_t s);
template <> int launch_bilateral_f32_joint_part<true, 3>(int radius, const BilateralF32Args& a, hipStream_t s);
template <> int launch_bilateral_f32_joint_part<false, 0>(int radius, const BilateralF32Args& a, hipStream_t s);
template <> int launch_bilateral_f32_joint_part<false, 1>(int radius, const BilateralF32Args& a, hipStream_t s);
template <> int launch_bilateral_f32_joint_part<false, 2>(int radius, const BilateralF32Args& a, hipStream_t s);
template <> int launch_bilateral_f32_joint_part<false, 3>(int radius, const BilateralF32Args& a, hipStream_t s);
template <bool FMA>
inline int launch_bilateral_f32_joint_fma(int radius, const BilateralF32Args& a, hipStream_t s) {
    if (radius < 0 || radius > kMaxRadius) return VIP_ERR_UNSUPPORTED_KSIZE;
    if (radius <= kBf32jPartHi[0]) return launch_bilateral_f32_joint_part<FMA, 0>(radius, a, s);
    if (radius <= kBf32jPartHi[1]) return launch_bilateral_f32_joint_part<FMA, 1>(radius, a, s);
    if (radius <= kBf32jPartHi[2]) return launch_bilateral_f32_joint_part<FMA, 2>(radius, a, s);
    return launch_bilateral_f32_joint_part<FMA, 3>(radius, a, s);
}
inline int launch_bilateral_f32_joint(int radius, bool fma, const BilateralF32Args& a, hipStream_t s) {
    return fma ? launch_bilateral_f32_joint_fma<true>(radius, a, s)
               : launch_bilateral_f32_joint_fma<false>(radius, a, s);
}
int launch_gradient_u8(const uint8_t* src, float* dst, int width, int height, int ch, hipStream_t stream);
int launch_gradient_f32(const float* src, float* dst, int width, int height, int ch, bool fma, hipStream_t stream);
int launch_blur_rtv(const uint8_t* img, const float* mag, float* blurred, float* rtv, int width, int height,
                    int ksize, bool cpp, hipStream_t stream);
int launch_guide(const float* blurred, const float* rtv, uint8_t* guide, int width, int height, int ksize, bool cpp,
                 hipStream_t stream);
int launch_texture_guide_fused(const uint8_t* img, uint8_t* guide, int width, int height, int ksize, bool cpp,
                               hipStream_t stream);
int launch_texture_guide_fused_rows(const uint8_t* img, uint8_t* guide, int width, int lo, int hi, int gy0, int gy1,
                                    int ksize, bool cpp, hipStream_t stream);
int launch_texture_iteration_fused(const StencilArgs& a, int ksize, bool cpp, hipStream_t stream);
// vip_gray_texture.hip: the fused guide stage on a one-channel frame (img: any base and pitch);
// rows [lo, hi) are valid, guide rows [gy0, gy1) inside them are produced
int launch_gray_texture_guide_rows(const uint8_t* img, size_t img_pitch, uint8_t* guide, size_t guide_pitch, int width,
                                   int lo, int hi, int gy0, int gy1, int ksize, bool cpp, hipStream_t stream);

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) once per kernel and device (the
// attribute is per device and one process may drive several). `devs` is the kernel's
// bitmask of devices done (ensure_lds owns it); concurrent first calls set it twice, which
// is harmless.
// ABS_LDS: the kernel addresses LDS absolutely (the SatLut tables: a constant byte offset
// in the ds_read immediate), which holds only while its dynamic LDS starts at byte 0, i.e.
// the kernel has no static LDS; checked once, a kernel with any is refused (hipErrorInvalidKernelFile).
inline int ensure_dynamic_lds(const void* kern, int bytes, std::atomic<unsigned long long>& devs, bool abs_lds) {
    int dev = 0;
    VIP_HIP_CHECK(hipGetDevice(&dev));
    const unsigned long long bit = 1ull << (dev & 63);
    if (devs.load(std::memory_order_relaxed) & bit) return 0;
    if (abs_lds) {
        hipFuncAttributes fa{};
        VIP_HIP_CHECK(hipFuncGetAttributes(&fa, kern));
        if (fa.sharedSizeBytes != 0) return (int)hipErrorInvalidKernelFile;
    }
    VIP_HIP_CHECK(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    devs.fetch_or(bit, std::memory_order_relaxed);
    return 0;
}
// The same, keyed by the kernel: each instantiation owns its kernel's device bitmask
// (static: a kernel is launched from one translation unit; no exported symbol per kernel)
template <auto KERN>
static int ensure_lds(int bytes, bool abs_lds = false) {
    static std::atomic<unsigned long long> devs{0};
    return ensure_dynamic_lds(reinterpret_cast<const void*>(KERN), bytes, devs, abs_lds);
}

// Launch log of the calling thread (vip_launched_kernels, vip_capi.hip): every stencil and
// texture-stage kernel notes its host stub before its launch, so a caller can name the
// exact template instantiation it timed (bench.py matches it against PMC summaries).
void note_launch(const void* kern);

// Kernel-duration recorder of the calling thread (vip_kernel_timing_*, vip_capi.hip): while
// it is on, the (start, stop) events for the next launch of `kern` on `stream`, else two
// nulls (also for a launch on another device than the recorder's, or into a stream that is
// being captured into a graph: its events would not be stamped).
struct LaunchEvents {
    hipEvent_t start, stop;
};
LaunchEvents timing_events(const void* kern, hipStream_t stream);

// Every stencil and texture launch goes through here: with the recorder on, the launch
// carries an event pair that the runtime stamps with the kernel's own begin and end
// (hipExtLaunchKernel: no marker packet enters the stream, so the duration is the one
// rocprofv3 --kernel-trace reports); otherwise a plain launch.
template <typename K, typename... Args>
inline void launch(K kern, dim3 grid, dim3 block, uint32_t lds, hipStream_t stream, Args... args) {
    const LaunchEvents ev = timing_events(reinterpret_cast<const void*>(kern), stream);
    if (ev.start)
        hipExtLaunchKernelGGL(kern, grid, block, lds, stream, ev.start, ev.stop, 0u, args...);
    else
        hipLaunchKernelGGL(kern, grid, block, lds, stream, args...);
}

// vip_bilateral_set_waves (vip_capi.hip): 0 = per-launch choice, else 16 / 8 / 4.
int bilateral_forced_waves();
// vip_bilateral_set_wide: 0 = per-launch choice, 1 = 128-pixel tiles (8 outputs per
// thread), 2 = 256-pixel tiles (4 outputs per thread, one row per wave).
int bilateral_forced_wide();

// One workgroup per CU of the current device (the 96 KiB LUT fills most of the CU's
// LDS), each striding over tiles; fewer blocks than CUs when the frame has fewer tiles.
inline int device_cus() {
    static std::atomic<int> cus_by_dev[64];  // CU count per device, 0 = not queried yet
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) dev = 0;
    int cus = cus_by_dev[dev & 63].load(std::memory_order_relaxed);
    if (cus == 0) {
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
            cus = 256;
        cus_by_dev[dev & 63].store(cus, std::memory_order_relaxed);
    }
    return cus;
}

// free_cus: CUs the launch leaves to concurrent work (StencilArgs::free_cus)
inline int persistent_blocks(int tiles, int free_cus = 0) {
    int cus = device_cus() - (free_cus > 0 ? free_cus : 0);
    cus = cus > 0 ? cus : 1;
    return tiles < cus ? tiles : cus;
}

// A persistent launch of T tiles on B workgroups runs ceil(T / B) rounds; when the last
// holds k = T mod B tiles, B - k workgroups idle through it while k run a whole tile each
// (a C2 slab batch at 8 GPUs: 1,530 tiles on 248 workgroups, 6.17 rounds run as 7). The
// last round's tiles are cut into m = 2^s pieces of WAVES / m waves each, the largest m
// with k * m <= B, so that k * m workgroups share them; a piece's workgroup still loads
// the whole tile plane (the apron rows its waves read) and its other waves skip the taps.
// m divides WAVES (a 12-wave tile is cut in 2 or 4, never 8). Returns s (0: no cut).
constexpr int tail_shift(int tiles, int blocks, int waves) {
    if (blocks <= 0 || tiles % blocks == 0) return 0;
    const long long k = tiles % blocks;
    int s = 0;
    while (waves % (2 << s) == 0 && (k << (s + 1)) <= blocks) ++s;
    return s;
}
static_assert(tail_shift(1530, 248, 16) == 2, "C2 slab batch at 8 GPUs: 42 tiles in 4 pieces");
static_assert(tail_shift(1530, 255, 16) == 0 && tail_shift(100, 100, 16) == 0, "even rounds: no cut");
static_assert(tail_shift(7 + 2 * 256, 256, 16) == 4 && tail_shift(7 + 2 * 256, 256, 12) == 2, "pieces divide WAVES");
static_assert(tail_shift(200 + 256, 256, 16) == 0, "k > blocks / 2: whole tiles");
inline void plan_tail(StencilArgs& a, int blocks, int waves) {
    const int s = tail_shift(a.tiles_total, blocks, waves);
    a.tail_full = s ? a.tiles_total - a.tiles_total % blocks : a.tiles_total;
    a.tail_shift = s;
}

// The launch of a persistent stencil kernel (bilateral, adaptive) once its tiling is chosen:
// KERN for one frame, FRAMES_KERN for a.nframes > 1 (nullptr: no multi-frame form, a.nframes
// is not looked at and the caller refuses such a launch), LDS bytes of dynamic LDS (ABS_LDS:
// see ensure_dynamic_lds), WAVES waves per workgroup, TW x TH pixel tiles. cut_tail: a
// multi-frame launch runs its last round in pieces (plan_tail). ARGS: the kernel's argument struct,
// StencilArgs or one derived from it (ConfArgs), copied whole.
template <auto KERN, auto FRAMES_KERN, int LDS, int WAVES, int TW, int TH, bool ABS_LDS, class ARGS>
static int launch_persistent(const ARGS& a, bool cut_tail, hipStream_t stream) {
    static_assert(std::is_base_of_v<StencilArgs, ARGS>, "kernel arguments");
    constexpr bool HAS_FRAMES = !std::is_null_pointer_v<decltype(FRAMES_KERN)>;
    const bool multi = HAS_FRAMES && a.nframes > 1;
    auto kern = KERN;
    int rc = 0;
    if constexpr (HAS_FRAMES) {
        if (multi) kern = FRAMES_KERN, rc = ensure_lds<FRAMES_KERN>(LDS, ABS_LDS);
    }
    if (!multi) rc = ensure_lds<KERN>(LDS, ABS_LDS);
    if (rc) return rc;
    note_launch(reinterpret_cast<const void*>(kern));
    ARGS args = a;
    args.tiles_x = (a.width + TW - 1) / TW;
    args.tiles_frame = args.tiles_x * ((a.out_rows + TH - 1) / TH);
    args.tiles_total = args.tiles_frame * (multi ? a.nframes : 1);
    if (args.tiles_total == 0) return 0;
    const int blocks = persistent_blocks(args.tiles_total, a.free_cus);
    args.tail_full = args.tiles_total;  // no cut: every item a whole tile on the XCD map
    args.tail_shift = 0;
    if (multi && cut_tail) plan_tail(args, blocks, WAVES);
    launch(kern, dim3(blocks), dim3(WAVES * 64), LDS, stream, args);
    return (int)hipGetLastError();
}

// The one-channel kernels' persistent launch: one frame, whole tiles of G::TW x WAVES * G::RPW
// pixels (G: the kernel's Geom), no absolute LDS address.
template <auto KERN, int LDS, int WAVES, class G, class ARGS>
static int launch_c1_tiles(const ARGS& a, hipStream_t stream) {
    static_assert(LDS <= kLdsBudget, "tile does not fit LDS");
    return launch_persistent<KERN, nullptr, LDS, WAVES, G::TW, WAVES * G::RPW, false>(a, false, stream);
}

// A run-time radius as a compile-time one: f(std::integral_constant<int, R>) for radius R in
// 1..kMaxRadius (every R is instantiated, in ascending order), VIP_ERR_UNSUPPORTED_KSIZE otherwise.
template <class F>
static int dispatch_radius(int radius, F&& f) {
    int rc = VIP_ERR_UNSUPPORTED_KSIZE;
    [&]<int... I>(std::integer_sequence<int, I...>) {
        (void)(... || (radius == I + 1 && (rc = f(std::integral_constant<int, I + 1>{}), true)));
    }(std::make_integer_sequence<int, kMaxRadius>{});
    return rc;
}

}  // namespace vip
