// extern "C" ABI of the MI355X bilateral-filter family (include/vip.h).
//
// Host-side responsibilities mirror the reference's Impl constructors
// (src/bilateral_filter_impl.cu:204-239, src/adaptive_bilateral_filter_impl.cu:117-152,
// src/bilateral_texture_filter_impl.cu:179-195): build the spatial and colour
// LUTs once per handle, own device scratch, validate arguments. Unlike the
// reference, run functions are asynchronous on the caller's stream and return a
// status instead of printing it.
#include <atomic>
#include <cmath>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <cxxabi.h>
#include <dlfcn.h>
#include <new>
#include <string>
#include <vector>

#include "vip_launch.hpp"

namespace vip {
// The templated kernel of a stencil filter (VIP_FILTER_BILATERAL, _JOINT or _ADAPTIVE)
static int launch_stencil(int filter, int radius, bool fma, const StencilArgs& a, hipStream_t s) {
    if (filter == VIP_FILTER_JOINT)
        return fma ? launch_bilateral_joint_fma(radius, a, s) : launch_bilateral_joint_mul(radius, a, s);
    if (filter == VIP_FILTER_ADAPTIVE) return fma ? launch_adaptive_fma(radius, a, s) : launch_adaptive_mul(radius, a, s);
    return fma ? launch_bilateral_plain_fma(radius, a, s) : launch_bilateral_plain_mul(radius, a, s);
}

// LUT construction. CUDA profile: src/bilateral_filter_impl.cu:217-237 (float
// coefficient, std::exp(float) == expf). CPP profile: include/cpp/bilateral_filter.hpp:13-36
// (double coefficient, exp, stored as float). `2 * sigma * sigma` is a float
// expression in both.
static float space_weight(int r2, float sigma_space, int numerics) {
    const float two_s2 = 2 * sigma_space * sigma_space;
    const float cf = -1.f / two_s2;
    const double cd = -1. / (double)two_s2;
    return numerics == VIP_NUMERICS_CPP ? (float)std::exp((double)r2 * cd) : expf((float)r2 * cf);
}

// Quadrant table ws[|ky|][|kx|] of the templated kernels (radius <= kMaxRadius)
static void build_space_q(int radius, float sigma_space, int numerics, float* wsq /* kWsStride^2 */) {
    for (int i = 0; i < kWsStride * kWsStride; ++i) wsq[i] = 0.f;
    if (radius > kMaxRadius) return;  // the runtime-radius kernel reads its own table
    for (int ky = 0; ky <= radius; ++ky)
        for (int kx = 0; kx <= radius; ++kx) {
            const int r2 = kx * kx + ky * ky;
            if (r2 > radius * radius) continue;
            wsq[ky * kWsStride + kx] = space_weight(r2, sigma_space, numerics);
        }
}

// Tables of the runtime-radius kernel (vip_stencil_rt.hip), one device allocation:
// (2R+1) rows of wst floats, row ky + R holding ws(kx, ky) at kx + ra for kx in
// [-ra, ra + 8) (zero outside the disc), then the R+1 disc half-widths as ints.
struct RtTables {
    float* d = nullptr;
    int wst = 0, ra = 0;
};
static int upload_rt_tables(int radius, float sigma_space, int numerics, RtTables* t) {
    t->ra = round_up(radius, 4);
    t->wst = 2 * t->ra + 8;
    const int rows = 2 * radius + 1;
    const size_t nf = (size_t)rows * t->wst;
    float* host = (float*)calloc(nf + radius + 1, sizeof(float));
    if (!host) return (int)hipErrorOutOfMemory;
    int* hw = reinterpret_cast<int*>(host + nf);
    for (int ky = -radius; ky <= radius; ++ky) {
        const int h = isqrt_floor(radius * radius - ky * ky);
        if (ky >= 0) hw[ky] = h;
        for (int kx = -h; kx <= h; ++kx)
            host[(size_t)(ky + radius) * t->wst + kx + t->ra] = space_weight(kx * kx + ky * ky, sigma_space, numerics);
    }
    const size_t bytes = (nf + radius + 1) * sizeof(float);
    int rc = (int)hipMalloc(reinterpret_cast<void**>(&t->d), bytes);
    if (!rc) rc = (int)hipMemcpy(t->d, host, bytes, hipMemcpyHostToDevice);
    free(host);
    return rc;
}

static void build_color(int len, float sigma_color, int numerics, float* out) {
    const float two_s2 = 2 * sigma_color * sigma_color;
    const float cf = -1.f / two_s2;
    const double cd = -1. / (double)two_s2;
    for (int i = 0; i < len; ++i)
        out[i] = numerics == VIP_NUMERICS_CPP ? (float)std::exp((double)(i * i) * cd) : expf((float)(i * i) * cf);
}

// The largest ksize the reference runs for each filter: its kernels size dynamic
// shared memory from ksize with no cap, against CUDA's 48 KB default
// (src/bilateral_filter_impl.cu:252-254 and :272-275, src/adaptive_bilateral_filter_impl.cu:165-167;
// the texture filter's JBF is ksize 2k-1, src/bilateral_texture_filter_impl.cu:188).
// Even ksizes stay rejected: the reference sizes its tile for ksize - 1 halo columns but
// reads 2 * (ksize / 2), past the tile.
constexpr int kMaxKsizeBilateral = 65, kMaxKsizeJoint = 47, kMaxKsizeAdaptive = 63, kMaxKsizeTexture = 24;
// joint bilateral upsampling has no reference counterpart: its ksize counts low-resolution pixels
constexpr int kMaxKsizeUpsample = 2 * kUpMaxRadius + 1;
// the confidence-weighted f32 joint filter has the radius-specialised kernels only (three LDS planes)
constexpr int kMaxKsizeJointConf = 2 * kMaxRadius + 1;
// the multi-channel f32 joint filter likewise (C + 1 LDS planes): by channel count, index 0 unused;
// one channel is the f32 joint filter itself
constexpr int kMaxKsizeJointF32c[5] = {0, kMaxKsizeJoint, 31, 15, 15};
// the self-guided f32 bilateral has the radius-specialised kernels only (vip_bilateral_f32_max_ksize)
constexpr int kMaxKsizeBilateralF32 = 2 * kMaxRadius + 1;
static bool valid_ksize(int ksize, int max_ksize) { return ksize >= 1 && (ksize & 1) && ksize <= max_ksize; }

// vip_set_stencil_path: VIP_PATH_AUTO (templated kernels for radius 1..15, the
// runtime-radius kernel for 0 and 16..32) or VIP_PATH_RUNTIME (the runtime-radius
// kernel for every radius; a test and measurement knob). Process-wide.
static std::atomic<int> g_stencil_path{[] {
    const char* e = getenv("VIP_STENCIL_PATH");
    return e && atoi(e) == VIP_PATH_RUNTIME ? VIP_PATH_RUNTIME : VIP_PATH_AUTO;
}()};
static bool use_runtime_kernel(int radius) {
    return radius == 0 || radius > kMaxRadius || g_stencil_path.load(std::memory_order_relaxed) == VIP_PATH_RUNTIME;
}

// Returns the number of leading entries up to the last nonzero one in *nonzero.
static int upload_color(float** d_color, int len, float sigma_color, int numerics, int* nonzero) {
    float host[1536];
    build_color(len, sigma_color, numerics, host);
    int nz = len;
    while (nz > 0 && host[nz - 1] == 0.f) --nz;
    *nonzero = nz;
    VIP_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(d_color), sizeof(float) * len));
    VIP_HIP_CHECK(hipMemcpy(*d_color, host, sizeof(float) * len, hipMemcpyHostToDevice));
    return 0;
}

// What the bilateral and adaptive handles share (vip_bilateral_s, vip_adaptive_s below)
struct StencilHandle {
    int width, height, ksize, radius, numerics, lut_nonzero;
    float* d_color;
    RtTables rt;  // runtime-radius kernel tables
    float wsq[kWsStride * kWsStride];
};

// A band of rows as the *_run_rows entry points take it: output rows [0, out_rows) of dst are
// source rows [src_row0, src_row0 + out_rows); every read clamps into rows [row_lo, row_hi).
struct RowBand {
    const uint8_t* src;
    size_t src_pitch;
    const uint8_t* guide;  // null: a plain filter
    size_t guide_pitch;
    uint8_t* dst;
    size_t dst_pitch;
    int out_rows, src_row0, row_lo, row_hi;
    // the plain filters' kernels read the source as their guide: said here, nowhere else
    const uint8_t* guide_or_src() const { return guide ? guide : src; }
    size_t guide_or_src_pitch() const { return guide ? guide_pitch : src_pitch; }
};

// src (and guide) hold the handle's height rows: every read clamps into [row_lo, row_hi),
// so that range must lie inside them
static bool rows_ok(int height, int out_rows, int row_lo, int row_hi) {
    return out_rows >= 0 && row_lo >= 0 && row_hi <= height && row_lo < row_hi;
}
static int check_band(int height, const RowBand& b) {
    if (!b.src || !b.dst || !rows_ok(height, b.out_rows, b.row_lo, b.row_hi)) return VIP_ERR_INVALID_ARGUMENT;
    if (b.dst == b.src || b.dst == b.guide_or_src()) return VIP_ERR_ALIASING;
    return 0;
}

static bool is_aligned(const void* p, size_t pitch, size_t to) { return (uintptr_t)p % to == 0 && pitch % to == 0; }
// Destination alignment that lets a kernel store a thread's outputs as whole words: the
// templated kernels write 8 outputs (24 bytes) as three qwords, the runtime-radius kernel
// 4 outputs (12 bytes) as three dwords (vip_stencil.hpp store_px_to)
constexpr size_t kStencilDstAlign = 8, kRtDstAlign = 4;

// The fields StencilArgs and RtArgs share: the band, and which accesses may be whole words
template <class Args>
static void band_args(Args& a, const StencilHandle& h, const RowBand& b, size_t dst_align) {
    a.src = b.src;
    a.guide = b.guide_or_src();
    a.dst = b.dst;
    a.src_pitch = (long long)b.src_pitch;
    a.guide_pitch = (long long)b.guide_or_src_pitch();
    a.dst_pitch = (long long)b.dst_pitch;
    a.width = h.width;
    a.out_rows = b.out_rows;
    a.src_row0 = b.src_row0;
    a.row_lo = b.row_lo;
    a.row_hi = b.row_hi;
    a.aligned = is_aligned(b.src, b.src_pitch, 4) && is_aligned(a.guide, b.guide_or_src_pitch(), 4);
    a.dst_aligned = is_aligned(b.dst, b.dst_pitch, dst_align);
    a.color = h.d_color;
}

// One frame's band for the templated kernels; `fold`: the joint kernel's folded tables or null
static StencilArgs stencil_args(const StencilHandle& h, const RowBand& b, const float* fold = nullptr) {
    StencilArgs a;
    band_args(a, h, b, kStencilDstAlign);
    a.tiles_x = (h.width + kTW - 1) / kTW;
    a.lut_nonzero = h.lut_nonzero;
    a.fold = fold;
    a.inflight = 1;
    a.nframes = 1;
    a.tiles_frame = 0;
    a.free_cus = 0;
    a.tail_full = 0;  // set per launch (launch_persistent: tiles_total, or plan_tail)
    a.tail_shift = 0;
    for (int f = 0; f < kMaxBatchFrames; ++f) {
        a.fsrc[f] = b.src;
        a.fdst[f] = b.dst;
    }
    std::memcpy(a.ws, h.wsq, sizeof(a.ws));
    return a;
}

static RtArgs rt_args(const StencilHandle& h, const RowBand& b) {
    RtArgs a{};
    band_args(a, h, b, kRtDstAlign);
    a.wsrow = h.rt.d;
    a.hw = reinterpret_cast<const int*>(h.rt.d + (size_t)(2 * h.radius + 1) * h.rt.wst);
    a.R = h.radius;
    a.wst = h.rt.wst;
    a.ra = h.rt.ra;
    return a;
}

// Frames in flight on the current device, for the plain bilateral kernel's small-frame
// tiling: the distinct streams among the device's last 8 plain-bilateral launches, at most
// 4 (the hardware queues a process gets by default, GPU_MAX_HW_QUEUES). One stream counts
// 1. The count is of streams, not of launches outstanding: a caller that alternates two
// streams but waits for each frame before the next also counts 2 (and gets the throughput
// tiling, e.g. C1's 14.5 instead of 10.7 us for a lone 512 x 512 frame), and after a change
// of streams the ring keeps the old count for up to 8 launches. Such a caller fixes the
// count with vip_bilateral_set_frames_in_flight(1). (Checking each recorded stream with
// hipStreamQuery would cost host time per launch and could touch a destroyed stream.) The
// choice changes the tiling only, never the bytes.
static std::atomic<int> g_bil_inflight{0};  // vip_bilateral_set_frames_in_flight: 0 = counted
static int frames_in_flight(hipStream_t s) {
    constexpr int kDevs = 16, kRing = 8;
    static std::atomic<uintptr_t> recent[kDevs][kRing];
    static std::atomic<unsigned> pos[kDevs];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) dev = 0;
    dev &= kDevs - 1;
    recent[dev][pos[dev].fetch_add(1, std::memory_order_relaxed) % kRing].store((uintptr_t)s + 1,
                                                                                 std::memory_order_relaxed);
    uintptr_t seen[kRing];
    int n = 0;
    for (int i = 0; i < kRing; ++i) {
        const uintptr_t v = recent[dev][i].load(std::memory_order_relaxed);
        bool dup = v == 0;
        for (int j = 0; j < n && !dup; ++j) dup = seen[j] == v;
        if (!dup) seen[n++] = v;
    }
    const int forced = g_bil_inflight.load(std::memory_order_relaxed);
    if (forced) return forced;
    return n < 1 ? 1 : (n > 4 ? 4 : n);
}

// vip_bilateral_set_waves: one process-wide value, read by every bilateral launcher
static bool valid_waves(int w) { return w == 0 || w == 16 || w == 8 || w == 4; }
static std::atomic<int> g_bil_waves{[] {
    const char* e = getenv("VIP_BIL_WAVES");
    const int w = e ? atoi(e) : 0;
    return valid_waves(w) ? w : 0;
}()};
int bilateral_forced_waves() { return g_bil_waves.load(std::memory_order_relaxed); }
static std::atomic<int> g_bil_wide{[] {
    const char* e = getenv("VIP_BIL_WIDE");
    const int w = e ? atoi(e) : 0;
    return w >= 0 && w <= 2 ? w : 0;
}()};
int bilateral_forced_wide() { return g_bil_wide.load(std::memory_order_relaxed); }

}  // namespace vip

using namespace vip;

struct vip_bilateral_s : StencilHandle {
    float* d_fold;  // joint kernel's folded tables (small sigma_color, radius <= kSatMaxR), or null
};

struct vip_adaptive_s : StencilHandle {};

// Joint bilateral upsampling: the frame, the scale and the two device tables. Read-only after
// create, so one handle serves any number of streams.
struct vip_upsample_s {
    int width, height, scale, radius, numerics, low_width, low_height;
    float* d_color;  // 768-entry colour LUT
    float* d_wsp;    // spatial weights (upload_upsample_space)
};

// Folded joint-kernel tables: table t (the t-th distinct r^2 of the disc, ascending)
// entry d = RN(ws(r^2) * wc[d]) for d < kFoldEntries -- the product the kernel's unfolded
// taps form (one float multiply), so results are unchanged. The kernel reads them behind
// the saturating address (SatLut) when wc is zero from its DZ on.
static int upload_fold(vip_bilateral_s* h, float sigma_color) {
    const int R = h->radius;
    float wc[768];
    build_color(768, sigma_color, h->numerics, wc);
    float fold[(kSatMaxR * kSatMaxR + 1) * kFoldEntries];
    int ntab = 0;
    for (int v = 0; v <= R * R; ++v) {
        if (!is_disc_r2(R, v)) continue;
        float ws = 0.f;  // the spatial weight of any tap at squared distance v
        for (int y = 0; y <= R; ++y)
            for (int x = 0; x <= R; ++x)
                if (x * x + y * y == v) ws = h->wsq[y * kWsStride + x];
        for (int d = 0; d < kFoldEntries; ++d) fold[ntab * kFoldEntries + d] = wc[d] * ws;
        ++ntab;
    }
    VIP_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&h->d_fold), sizeof(float) * kFoldEntries * ntab));
    VIP_HIP_CHECK(hipMemcpy(h->d_fold, fold, sizeof(float) * kFoldEntries * ntab, hipMemcpyHostToDevice));
    return 0;
}

// The two create functions: the geometry, the spatial tables, the colour LUT of lut_len
// entries, the runtime-radius tables and (bilateral) the folded tables
struct StencilSpec {
    int width, height, ksize;
    float sigma_space, sigma_color;
    int numerics;
};
template <class H>
static int destroy_stencil(H* h) {
    if (!h) return 0;
    if constexpr (std::is_same_v<H, vip_bilateral_s>)
        if (h->d_fold) (void)hipFree(h->d_fold);
    if (h->rt.d) (void)hipFree(h->rt.d);
    const int rc = h->d_color ? (int)hipFree(h->d_color) : 0;
    delete h;
    return rc;
}
template <class H>
static int create_stencil(H** out, const StencilSpec& p, int max_ksize, int lut_len) {
    if (!out || p.width <= 0 || p.height <= 0) return VIP_ERR_INVALID_ARGUMENT;
    if (!valid_ksize(p.ksize, max_ksize)) return VIP_ERR_UNSUPPORTED_KSIZE;
    H* h = new (std::nothrow) H();
    if (!h) return (int)hipErrorOutOfMemory;
    h->width = p.width;
    h->height = p.height;
    h->ksize = p.ksize;
    h->radius = p.ksize / 2;
    h->numerics = p.numerics == VIP_NUMERICS_CPP ? VIP_NUMERICS_CPP : VIP_NUMERICS_CUDA;
    build_space_q(h->radius, p.sigma_space, h->numerics, h->wsq);
    int rc = upload_color(&h->d_color, lut_len, p.sigma_color, h->numerics, &h->lut_nonzero);
    if (!rc) rc = upload_rt_tables(h->radius, p.sigma_space, h->numerics, &h->rt);
    if constexpr (std::is_same_v<H, vip_bilateral_s>)
        if (!rc && h->lut_nonzero < kFoldEntries && h->radius <= kSatMaxR) rc = upload_fold(h, p.sigma_color);
    if (rc) {
        destroy_stencil(h);
        return rc;
    }
    *out = h;
    return 0;
}

// The handle owns three u8x3 frames: the two ping-pong frames and the guide. The
// reference's Impl also holds f32 magnitude, blurred and rtv buffers
// (src/bilateral_texture_filter_impl.cu:189-194, 20 B/px); here the guide stage keeps
// them in LDS, and the stage entry points (vip_texture_blur_rtv / _guide) write the
// caller's buffers, so the handle holds none.
struct vip_texture_s {
    int width, height, ksize, nitr, numerics;
    int mode;  // VIP_TEXTURE_TWO_LAUNCH or VIP_TEXTURE_FUSED (vip_texture_set_mode)
    vip_bilateral_t jbf;
    uint8_t* d_ping[2];
    uint8_t* d_guide;
    // vip_texture_run_c1: the gray guide's colour table, entry d = entry 3d of the JBF's LUT
    // (three equal channels: L1 distance 3 |G_n - G_c|), and its leading nonzero entries
    float* d_color_c1;
    int lut_nonzero_c1;
};

namespace {
thread_local const void* g_launched[16];  // distinct kernels launched since the last query
thread_local int g_nlaunched = 0;

// vip_kernel_timing_*: a per-thread pool of event pairs on one device, the kernel of each
// recorded launch, and how many of the `cap` slots are used
struct KernelTiming {
    std::vector<hipEvent_t> ev;  // 2 per slot: start, stop
    std::vector<const void*> kern;
    int device = -1, cap = 0, n = 0;
    bool on = false;
    ~KernelTiming() {
        for (hipEvent_t e : ev) (void)hipEventDestroy(e);
    }
};
thread_local KernelTiming g_timing;

// The profiler's name of a kernel handle: the exported symbol's mangled name (dladdr; the
// runtime's lookup is the fallback), demangled, without the parameter list.
std::string kernel_name(const void* kern) {
    Dl_info info{};
    const char* mangled = dladdr(kern, &info) && info.dli_sname && info.dli_saddr == kern
                              ? info.dli_sname
                              : hipKernelNameRefByPtr(kern, nullptr);
    if (!mangled) return {};
    int st = 0;
    char* dem = abi::__cxa_demangle(mangled, nullptr, nullptr, &st);
    std::string name = st == 0 && dem ? dem : mangled;
    std::free(dem);
    const size_t paren = name.find('(');
    if (paren != std::string::npos) name.resize(paren);  // the profiler summaries' key: no parameter list
    return name;
}
}  // namespace

namespace vip {
void note_launch(const void* kern) {
    for (int i = 0; i < g_nlaunched; ++i)
        if (g_launched[i] == kern) return;
    if (g_nlaunched < 16) g_launched[g_nlaunched++] = kern;
}

LaunchEvents timing_events(const void* kern, hipStream_t stream) {
    KernelTiming& t = g_timing;
    if (!t.on || t.n >= t.cap) return {nullptr, nullptr};
    int dev = -1;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipGetDevice(&dev) != hipSuccess || dev != t.device || hipStreamIsCapturing(stream, &cap) != hipSuccess ||
        cap != hipStreamCaptureStatusNone)
        return {nullptr, nullptr};
    t.kern[t.n] = kern;
    const int i = t.n++;
    return {t.ev[2 * i], t.ev[2 * i + 1]};
}
}  // namespace vip

extern "C" {

int vip_launched_kernels(char* buf, size_t len) {
    std::string all;
    for (int i = 0; i < g_nlaunched; ++i) {
        const std::string name = kernel_name(g_launched[i]);
        if (!name.empty()) all += (all.empty() ? "" : "\n") + name;
    }
    if (buf && len) {
        g_nlaunched = 0;  // a size query (no buffer) keeps the list
        const size_t n = all.size() < len - 1 ? all.size() : len - 1;
        std::memcpy(buf, all.data(), n);
        buf[n] = 0;
    }
    return (int)all.size();
}

int vip_kernel_timing_begin(int capacity) {
    if (capacity < 1 || capacity > (1 << 16)) return VIP_ERR_INVALID_ARGUMENT;
    KernelTiming& t = g_timing;
    int dev = 0;
    VIP_HIP_CHECK(hipGetDevice(&dev));
    if (dev != t.device) {  // events belong to the device current at their creation
        for (hipEvent_t e : t.ev) (void)hipEventDestroy(e);
        t.ev.clear();
        t.device = dev;
    }
    while ((int)t.ev.size() < 2 * capacity) {
        hipEvent_t e = nullptr;
        VIP_HIP_CHECK(hipEventCreate(&e));
        t.ev.push_back(e);
    }
    t.kern.assign((size_t)capacity, nullptr);
    t.cap = capacity;
    t.n = 0;
    t.on = true;
    return 0;
}

int vip_kernel_timing_end(void) {
    g_timing.on = false;
    return g_timing.n;
}

int vip_kernel_timing_get(int index, float* ms, char* name, size_t len) {
    KernelTiming& t = g_timing;
    if (index < 0 || index >= t.n || t.on || !ms) return VIP_ERR_INVALID_ARGUMENT;
    VIP_HIP_CHECK(hipEventSynchronize(t.ev[2 * index + 1]));
    VIP_HIP_CHECK(hipEventElapsedTime(ms, t.ev[2 * index], t.ev[2 * index + 1]));
    if (name && len) {
        const std::string s = kernel_name(t.kern[index]);
        const size_t n = s.size() < len - 1 ? s.size() : len - 1;
        std::memcpy(name, s.data(), n);
        name[n] = 0;
    }
    return 0;
}

int vip_abi_version(void) { return VIP_ABI_VERSION; }
int vip_max_radius(void) { return kRtMaxRadius; }

int vip_max_ksize(int filter) {
    switch (filter) {
        case VIP_FILTER_BILATERAL: return kMaxKsizeBilateral;
        case VIP_FILTER_JOINT: return kMaxKsizeJoint;
        case VIP_FILTER_ADAPTIVE: return kMaxKsizeAdaptive;
        case VIP_FILTER_TEXTURE: return kMaxKsizeTexture;
        case VIP_FILTER_UPSAMPLE: return kMaxKsizeUpsample;
        case VIP_FILTER_JOINT_CONF: return kMaxKsizeJointConf;
        case VIP_FILTER_JOINT_F32C: return kMaxKsizeJointF32c[2];
        default: return VIP_ERR_INVALID_ARGUMENT;
    }
}

int vip_joint_f32c_max_ksize(int channels) {
    return channels >= 1 && channels <= 4 ? kMaxKsizeJointF32c[channels] : VIP_ERR_INVALID_ARGUMENT;
}

int vip_set_stencil_path(int path) {
    if (path != VIP_PATH_AUTO && path != VIP_PATH_RUNTIME) return VIP_ERR_INVALID_ARGUMENT;
    g_stencil_path.store(path, std::memory_order_relaxed);
    return 0;
}

int vip_bilateral_set_waves(int waves) {
    if (!valid_waves(waves)) return VIP_ERR_INVALID_ARGUMENT;
    g_bil_waves.store(waves, std::memory_order_relaxed);
    return 0;
}

int vip_bilateral_set_wide(int mode) {
    if (mode < 0 || mode > 2) return VIP_ERR_INVALID_ARGUMENT;
    g_bil_wide.store(mode, std::memory_order_relaxed);
    return 0;
}

int vip_bilateral_set_frames_in_flight(int n) {
    if (n < 0 || n > 4) return VIP_ERR_INVALID_ARGUMENT;
    g_bil_inflight.store(n, std::memory_order_relaxed);
    return 0;
}

const char* vip_error_string(int code) {
    switch (code) {
        case 0: return "success";
        case VIP_ERR_INVALID_ARGUMENT: return "invalid argument";
        case VIP_ERR_UNSUPPORTED_KSIZE:
            return "unsupported ksize (odd, 1..65 bilateral, 1..47 joint bilateral, 1..63 adaptive, 1..9 upsampling, 1..31 confidence-weighted "
                   "joint, 1..31 / 1..15 joint on 2 / 3-4 f32 channels, 1..31 self-guided f32 bilateral; texture 1..24)";
        case VIP_ERR_ALIASING: return "source and destination alias";
        default: return hipGetErrorString((hipError_t)code);
    }
}

int vip_malloc(void** d_ptr, size_t bytes) {
    if (!d_ptr) return VIP_ERR_INVALID_ARGUMENT;
    return (int)hipMalloc(d_ptr, bytes);
}
int vip_free(void* d_ptr) { return (int)hipFree(d_ptr); }
int vip_upload(void* d_dst, const void* h_src, size_t bytes) {
    return (int)hipMemcpy(d_dst, h_src, bytes, hipMemcpyHostToDevice);
}
int vip_download(void* h_dst, const void* d_src, size_t bytes) {
    return (int)hipMemcpy(h_dst, d_src, bytes, hipMemcpyDeviceToHost);
}
int vip_device_synchronize(void) { return (int)hipDeviceSynchronize(); }
int vip_device_count(int* count) {
    if (!count) return VIP_ERR_INVALID_ARGUMENT;
    return (int)hipGetDeviceCount(count);
}
int vip_set_device(int device) { return (int)hipSetDevice(device); }
int vip_get_device(int* device) {
    if (!device) return VIP_ERR_INVALID_ARGUMENT;
    return (int)hipGetDevice(device);
}
int vip_stream_synchronize(void* stream) { return (int)hipStreamSynchronize((hipStream_t)stream); }
int vip_host_alloc(void** h_ptr, size_t bytes) {
    if (!h_ptr) return VIP_ERR_INVALID_ARGUMENT;
    return (int)hipHostMalloc(h_ptr, bytes, hipHostMallocDefault);
}
int vip_host_free(void* h_ptr) { return (int)hipHostFree(h_ptr); }
int vip_upload_async(void* d_dst, const void* h_src, size_t bytes, void* stream) {
    return (int)hipMemcpyAsync(d_dst, h_src, bytes, hipMemcpyHostToDevice, (hipStream_t)stream);
}
int vip_download_async(void* h_dst, const void* d_src, size_t bytes, void* stream) {
    return (int)hipMemcpyAsync(h_dst, d_src, bytes, hipMemcpyDeviceToHost, (hipStream_t)stream);
}
int vip_stream_create(void** stream) {
    if (!stream) return VIP_ERR_INVALID_ARGUMENT;
    return (int)hipStreamCreateWithFlags(reinterpret_cast<hipStream_t*>(stream), hipStreamNonBlocking);
}
int vip_stream_destroy(void* stream) { return (int)hipStreamDestroy((hipStream_t)stream); }
int vip_event_create(void** event) {
    if (!event) return VIP_ERR_INVALID_ARGUMENT;
    return (int)hipEventCreateWithFlags(reinterpret_cast<hipEvent_t*>(event), hipEventDisableTiming);
}
int vip_event_destroy(void* event) { return (int)hipEventDestroy((hipEvent_t)event); }
int vip_event_record(void* event, void* stream) { return (int)hipEventRecord((hipEvent_t)event, (hipStream_t)stream); }
int vip_stream_wait_event(void* stream, void* event) {
    return (int)hipStreamWaitEvent((hipStream_t)stream, (hipEvent_t)event, 0);
}
int vip_event_synchronize(void* event) { return (int)hipEventSynchronize((hipEvent_t)event); }

// ---------------------------------------------------------------- bilateral
int vip_bilateral_create(vip_bilateral_t* out, int width, int height, int ksize, float sigma_space, float sigma_color,
                         int numerics) {
    return create_stencil(out, {width, height, ksize, sigma_space, sigma_color, numerics}, kMaxKsizeBilateral, 768);
}

int vip_bilateral_destroy(vip_bilateral_t h) { return destroy_stencil(h); }

// One band through a stencil filter of handle h: the runtime-radius kernel or the
// templated one. `fold`: the joint filter's folded tables, or null.
static int run_band(const StencilHandle& h, int filter, const RowBand& b, const float* fold, hipStream_t s) {
    const bool fma = h.numerics == VIP_NUMERICS_CUDA;
    if (use_runtime_kernel(h.radius))
        return launch_stencil_rt(rt_args(h, b), filter == VIP_FILTER_JOINT, filter == VIP_FILTER_ADAPTIVE, fma, s);
    StencilArgs a = stencil_args(h, b, fold);
    if (filter == VIP_FILTER_BILATERAL) a.inflight = frames_in_flight(s);
    return launch_stencil(filter, h.radius, fma, a, s);
}

int vip_bilateral_run_rows(vip_bilateral_t h, const uint8_t* d_src, size_t src_pitch, const uint8_t* d_guide,
                           size_t guide_pitch, uint8_t* d_dst, size_t dst_pitch, int out_rows, int src_row0,
                           int row_lo, int row_hi, void* stream) {
    if (!h) return VIP_ERR_INVALID_ARGUMENT;
    const RowBand b{d_src, src_pitch, d_guide, guide_pitch, d_dst, dst_pitch, out_rows, src_row0, row_lo, row_hi};
    if (const int rc = check_band(h->height, b)) return rc;
    const bool joint = d_guide != nullptr;
    if (joint && h->ksize > kMaxKsizeJoint) return VIP_ERR_UNSUPPORTED_KSIZE;
    return run_band(*h, joint ? VIP_FILTER_JOINT : VIP_FILTER_BILATERAL, b, joint ? h->d_fold : nullptr,
                    (hipStream_t)stream);
}

// ---- single-channel forms (vip_gray.hip): the same band, handle and tables; guide_channels 0
// plain, 1 or 3 joint
int vip_bilateral_run_rows_c1(vip_bilateral_t h, const uint8_t* d_src, size_t src_pitch, const uint8_t* d_guide,
                              size_t guide_pitch, int guide_channels, uint8_t* d_dst, size_t dst_pitch, int out_rows,
                              int src_row0, int row_lo, int row_hi, void* stream) {
    if (!h) return VIP_ERR_INVALID_ARGUMENT;
    const RowBand b{d_src, src_pitch, d_guide, guide_pitch, d_dst, dst_pitch, out_rows, src_row0, row_lo, row_hi};
    if (const int rc = check_band(h->height, b)) return rc;
    const bool joint = d_guide != nullptr;
    if (joint && guide_channels != 1 && guide_channels != 3) return VIP_ERR_INVALID_ARGUMENT;
    if (joint && h->ksize > kMaxKsizeJoint) return VIP_ERR_UNSUPPORTED_KSIZE;
    const int gch = joint ? guide_channels : 0;
    const bool fma = h->numerics == VIP_NUMERICS_CUDA;
    if (use_runtime_kernel(h->radius)) return launch_gray_rt(rt_args(*h, b), gch, fma, (hipStream_t)stream);
    return launch_gray(h->radius, gch, fma, stencil_args(*h, b), (hipStream_t)stream);
}

int vip_bilateral_run_c1(vip_bilateral_t h, const uint8_t* d_src, size_t src_pitch, uint8_t* d_dst, size_t dst_pitch,
                         void* stream) {
    if (!h) return VIP_ERR_INVALID_ARGUMENT;
    return vip_bilateral_run_rows_c1(h, d_src, src_pitch, nullptr, 0, 0, d_dst, dst_pitch, h->height, 0, 0, h->height,
                                     stream);
}

int vip_joint_bilateral_run_c1(vip_bilateral_t h, const uint8_t* d_src, size_t src_pitch, const uint8_t* d_guide,
                               size_t guide_pitch, int guide_channels, uint8_t* d_dst, size_t dst_pitch,
                               void* stream) {
    if (!h || !d_guide) return VIP_ERR_INVALID_ARGUMENT;
    return vip_bilateral_run_rows_c1(h, d_src, src_pitch, d_guide, guide_pitch, guide_channels, d_dst, dst_pitch,
                                     h->height, 0, 0, h->height, stream);
}

// ---- f32 one-channel source under an 8-bit guide (vip_joint_f32.hip): the same band, handle and
// tables; the float pointers travel as the band's byte pointers, and the flags that pick the
// wide loads and stores take the meanings the f32 kernels give them
int vip_joint_bilateral_run_rows_f32(vip_bilateral_t h, const float* d_src, size_t src_pitch, const uint8_t* d_guide,
                                     size_t guide_pitch, int guide_channels, float* d_dst, size_t dst_pitch,
                                     int out_rows, int src_row0, int row_lo, int row_hi, void* stream) {
    if (!h || !d_guide) return VIP_ERR_INVALID_ARGUMENT;
    const RowBand b{reinterpret_cast<const uint8_t*>(d_src), src_pitch, d_guide, guide_pitch,
                    reinterpret_cast<uint8_t*>(d_dst), dst_pitch, out_rows, src_row0, row_lo, row_hi};
    if (const int rc = check_band(h->height, b)) return rc;
    if (guide_channels != 1 && guide_channels != 3) return VIP_ERR_INVALID_ARGUMENT;
    if (!is_aligned(d_src, src_pitch, 4) || !is_aligned(d_dst, dst_pitch, 4)) return VIP_ERR_INVALID_ARGUMENT;
    if (h->ksize > kMaxKsizeJoint) return VIP_ERR_UNSUPPORTED_KSIZE;
    const int aligned = (is_aligned(d_guide, guide_pitch, 4) ? kF32GuideWords : 0) |
                        (is_aligned(d_src, src_pitch, 16) ? kF32SrcVec : 0);
    const int dst_aligned = is_aligned(d_dst, dst_pitch, 16);
    const bool fma = h->numerics == VIP_NUMERICS_CUDA;
    if (use_runtime_kernel(h->radius)) {
        RtArgs a = rt_args(*h, b);
        a.aligned = aligned;
        a.dst_aligned = dst_aligned;
        return launch_joint_f32_rt(a, guide_channels, fma, (hipStream_t)stream);
    }
    StencilArgs a = stencil_args(*h, b);
    a.aligned = aligned;
    a.dst_aligned = dst_aligned;
    return launch_joint_f32(h->radius, guide_channels, fma, a, (hipStream_t)stream);
}

int vip_joint_bilateral_run_f32(vip_bilateral_t h, const float* d_src, size_t src_pitch, const uint8_t* d_guide,
                                size_t guide_pitch, int guide_channels, float* d_dst, size_t dst_pitch,
                                void* stream) {
    if (!h) return VIP_ERR_INVALID_ARGUMENT;
    return vip_joint_bilateral_run_rows_f32(h, d_src, src_pitch, d_guide, guide_pitch, guide_channels, d_dst,
                                            dst_pitch, h->height, 0, 0, h->height, stream);
}

// ---- confidence-weighted form of the f32 joint filter (vip_joint_conf.hip): the whole frame, the
// radius-specialised kernels only; each float array's 16-byte accesses are decided on its own
int vip_joint_bilateral_run_conf_f32(vip_bilateral_t h, const float* d_src, size_t src_pitch, const float* d_conf,
                                     size_t conf_pitch, const uint8_t* d_guide, size_t guide_pitch,
                                     int guide_channels, float hole_value, float* d_dst, size_t dst_pitch,
                                     float* d_weight, size_t weight_pitch, void* stream) {
    if (!h || !d_src || !d_conf || !d_guide || !d_dst) return VIP_ERR_INVALID_ARGUMENT;
    if (guide_channels != 1 && guide_channels != 3) return VIP_ERR_INVALID_ARGUMENT;
    if (!is_aligned(d_src, src_pitch, 4) || !is_aligned(d_conf, conf_pitch, 4) || !is_aligned(d_dst, dst_pitch, 4) ||
        (d_weight && !is_aligned(d_weight, weight_pitch, 4)))
        return VIP_ERR_INVALID_ARGUMENT;
    const size_t frow = sizeof(float) * (size_t)h->width;
    if (src_pitch < frow || conf_pitch < frow || dst_pitch < frow || (d_weight && weight_pitch < frow) ||
        guide_pitch < (size_t)guide_channels * (size_t)h->width)
        return VIP_ERR_INVALID_ARGUMENT;
    const void* const ins[3] = {d_src, d_conf, d_guide};
    for (const void* in : ins)
        if (in == d_dst || in == d_weight) return VIP_ERR_ALIASING;
    if (d_dst == d_weight) return VIP_ERR_ALIASING;
    if (h->ksize > kMaxKsizeJointConf) return VIP_ERR_UNSUPPORTED_KSIZE;
    const RowBand b{reinterpret_cast<const uint8_t*>(d_src), src_pitch, d_guide, guide_pitch,
                    reinterpret_cast<uint8_t*>(d_dst), dst_pitch, h->height, 0, 0, h->height};
    ConfArgs a;
    static_cast<StencilArgs&>(a) = stencil_args(*h, b);
    a.aligned = (is_aligned(d_guide, guide_pitch, 4) ? kF32GuideWords : 0) |
                (is_aligned(d_src, src_pitch, 16) ? kF32SrcVec : 0);
    a.dst_aligned = is_aligned(d_dst, dst_pitch, 16);
    a.conf = reinterpret_cast<const uint8_t*>(d_conf);
    a.conf_pitch = (long long)conf_pitch;
    a.conf_vec = is_aligned(d_conf, conf_pitch, 16);
    a.weight = reinterpret_cast<uint8_t*>(d_weight);
    a.weight_pitch = (long long)weight_pitch;
    a.weight_aligned = d_weight && is_aligned(d_weight, weight_pitch, 16);
    a.hole_value = hole_value;
    return launch_joint_conf_f32(h->radius, guide_channels, h->numerics == VIP_NUMERICS_CUDA, a, (hipStream_t)stream);
}

// ---- the f32 joint filter on an interleaved source of 2..4 channels (vip_joint_f32c.hip): the whole
// frame, the radius-specialised kernels only; a row is width * channels floats, and the 16-byte
// accesses are decided for src and dst each on its own
int vip_joint_bilateral_run_f32c(vip_bilateral_t h, const float* d_src, size_t src_pitch, int channels,
                                 const uint8_t* d_guide, size_t guide_pitch, int guide_channels, float* d_dst,
                                 size_t dst_pitch, void* stream) {
    if (!h || !d_src || !d_guide || !d_dst) return VIP_ERR_INVALID_ARGUMENT;
    if (channels < 1 || channels > 4) return VIP_ERR_INVALID_ARGUMENT;
    if (channels == 1)
        return vip_joint_bilateral_run_f32(h, d_src, src_pitch, d_guide, guide_pitch, guide_channels, d_dst, dst_pitch,
                                           stream);
    if (guide_channels != 1 && guide_channels != 3) return VIP_ERR_INVALID_ARGUMENT;
    if (!is_aligned(d_src, src_pitch, 4) || !is_aligned(d_dst, dst_pitch, 4)) return VIP_ERR_INVALID_ARGUMENT;
    const size_t frow = sizeof(float) * (size_t)channels * (size_t)h->width;
    if (src_pitch < frow || dst_pitch < frow || guide_pitch < (size_t)guide_channels * (size_t)h->width)
        return VIP_ERR_INVALID_ARGUMENT;
    if (d_dst == d_src || (const void*)d_dst == (const void*)d_guide) return VIP_ERR_ALIASING;
    if (h->ksize > kMaxKsizeJointF32c[channels]) return VIP_ERR_UNSUPPORTED_KSIZE;
    const RowBand b{reinterpret_cast<const uint8_t*>(d_src), src_pitch, d_guide, guide_pitch,
                    reinterpret_cast<uint8_t*>(d_dst), dst_pitch, h->height, 0, 0, h->height};
    StencilArgs a = stencil_args(*h, b);
    a.aligned = (is_aligned(d_guide, guide_pitch, 4) ? kF32GuideWords : 0) |
                (is_aligned(d_src, src_pitch, 16) ? kF32SrcVec : 0);
    a.dst_aligned = is_aligned(d_dst, dst_pitch, 16);
    const bool fma = h->numerics == VIP_NUMERICS_CUDA;
    return launch_joint_f32c(h->radius, channels, guide_channels, fma, a, (hipStream_t)stream);
}

// ---- self-guided f32 bilateral (vip_bilateral_f32.hpp): a handle of its own, since the range
// table depends on value_range. The StencilHandle part carries the geometry, the spatial table
// and, as d_color, the device table of kBf32Pairs (L[i], D[i]) pairs; it has no runtime-radius tables.
struct vip_bilateral_f32_s : StencilHandle {
    float scale;
};

int vip_bilateral_f32_max_ksize(void) { return kMaxKsizeBilateralF32; }

int vip_bilateral_f32_create(vip_bilateral_f32_t* out, int width, int height, int ksize, float sigma_space,
                             float sigma_color, float value_range, int numerics) {
    constexpr int N = VIP_BILATERAL_F32_BINS;
    if (!out || width <= 0 || height <= 0) return VIP_ERR_INVALID_ARGUMENT;
    if (!std::isfinite(value_range) || !(value_range > 0.f)) return VIP_ERR_INVALID_ARGUMENT;
    const float scale = (float)N / value_range;
    if (!std::isfinite(scale) || !(scale > 0.f)) return VIP_ERR_INVALID_ARGUMENT;
    if (!valid_ksize(ksize, kMaxKsizeBilateralF32)) return VIP_ERR_UNSUPPORTED_KSIZE;
    vip_bilateral_f32_s* h = new (std::nothrow) vip_bilateral_f32_s();
    if (!h) return (int)hipErrorOutOfMemory;
    h->width = width;
    h->height = height;
    h->ksize = ksize;
    h->radius = ksize / 2;
    h->numerics = numerics == VIP_NUMERICS_CPP ? VIP_NUMERICS_CPP : VIP_NUMERICS_CUDA;
    h->lut_nonzero = 0;
    h->scale = scale;
    build_space_q(h->radius, sigma_space, h->numerics, h->wsq);
    // the range table: L at the differences i / scale (build_color's coefficients), its slopes beside it
    const float two_s2 = 2 * sigma_color * sigma_color;
    const float cf = -1.f / two_s2;
    const double cd = -1. / (double)two_s2;
    std::vector<float> L(N + 2), pairs(2 * (size_t)kBf32Pairs);
    for (int i = 0; i <= N; ++i) {
        const float v = (float)i / scale;
        L[i] = h->numerics == VIP_NUMERICS_CPP ? (float)std::exp((double)v * (double)v * cd) : expf((v * v) * cf);
    }
    L[N + 1] = L[N];
    for (int i = 0; i <= N; ++i) {
        pairs[2 * i] = L[i];
        pairs[2 * i + 1] = L[i + 1] - L[i];
    }
    int rc = (int)hipMalloc(reinterpret_cast<void**>(&h->d_color), sizeof(float) * pairs.size());
    if (!rc) rc = (int)hipMemcpy(h->d_color, pairs.data(), sizeof(float) * pairs.size(), hipMemcpyHostToDevice);
    if (rc) {
        vip_bilateral_f32_destroy(h);
        return rc;
    }
    *out = h;
    return 0;
}

int vip_bilateral_f32_destroy(vip_bilateral_f32_t h) {
    if (!h) return 0;
    const int rc = h->d_color ? (int)hipFree(h->d_color) : 0;
    delete h;
    return rc;
}

int vip_bilateral_f32_run_rows(vip_bilateral_f32_t h, const float* d_src, size_t src_pitch, float* d_dst,
                               size_t dst_pitch, int out_rows, int src_row0, int row_lo, int row_hi,
                               void* stream) {
    if (!h) return VIP_ERR_INVALID_ARGUMENT;
    const RowBand b{reinterpret_cast<const uint8_t*>(d_src), src_pitch, nullptr, 0,
                    reinterpret_cast<uint8_t*>(d_dst), dst_pitch, out_rows, src_row0, row_lo, row_hi};
    if (const int rc = check_band(h->height, b)) return rc;
    if (!is_aligned(d_src, src_pitch, 4) || !is_aligned(d_dst, dst_pitch, 4)) return VIP_ERR_INVALID_ARGUMENT;
    BilateralF32Args a;
    static_cast<StencilArgs&>(a) = stencil_args(*h, b);
    a.aligned = is_aligned(d_src, src_pitch, 16) ? kF32SrcVec : 0;
    a.dst_aligned = is_aligned(d_dst, dst_pitch, 16);
    a.scale = h->scale;
    return launch_bilateral_f32(h->radius, h->numerics == VIP_NUMERICS_CUDA, a, (hipStream_t)stream);
}

int vip_bilateral_f32_run(vip_bilateral_f32_t h, const float* d_src, size_t src_pitch, float* d_dst,
                          size_t dst_pitch, void* stream) {
    if (!h) return VIP_ERR_INVALID_ARGUMENT;
    return vip_bilateral_f32_run_rows(h, d_src, src_pitch, d_dst, dst_pitch, h->height, 0, 0, h->height, stream);
}

// ---- the self-guided f32 bilateral on an interleaved image of 2 or 3 channels (vip_bilateral_f32c.hpp):
// the same handle, tables and band; a row is width * channels floats, the 16-byte accesses are
// decided for src and dst each on its own, and channels == 1 is the one-channel entry point itself
constexpr int kMaxKsizeBilateralF32c[4] = {0, kMaxKsizeBilateralF32, 2 * kBf32cMaxRadius + 1, 2 * kBf32cMaxRadius + 1};

int vip_bilateral_f32_max_ksize_c(int channels) {
    return channels >= 1 && channels <= 3 ? kMaxKsizeBilateralF32c[channels] : 0;
}

int vip_bilateral_f32_run_rows_c(vip_bilateral_f32_t h, const float* d_src, size_t src_pitch, int channels,
                                 float* d_dst, size_t dst_pitch, int out_rows, int src_row0, int row_lo, int row_hi,
                                 void* stream) {
    if (channels < 1 || channels > 3) return VIP_ERR_INVALID_ARGUMENT;
    if (channels == 1)
        return vip_bilateral_f32_run_rows(h, d_src, src_pitch, d_dst, dst_pitch, out_rows, src_row0, row_lo, row_hi,
                                          stream);
    if (!h) return VIP_ERR_INVALID_ARGUMENT;
    const RowBand b{reinterpret_cast<const uint8_t*>(d_src), src_pitch, nullptr, 0,
                    reinterpret_cast<uint8_t*>(d_dst), dst_pitch, out_rows, src_row0, row_lo, row_hi};
    if (const int rc = check_band(h->height, b)) return rc;
    if (!is_aligned(d_src, src_pitch, 4) || !is_aligned(d_dst, dst_pitch, 4)) return VIP_ERR_INVALID_ARGUMENT;
    const size_t frow = sizeof(float) * (size_t)channels * (size_t)h->width;
    if (src_pitch < frow || dst_pitch < frow) return VIP_ERR_INVALID_ARGUMENT;
    if (h->ksize > kMaxKsizeBilateralF32c[channels]) return VIP_ERR_UNSUPPORTED_KSIZE;
    BilateralF32Args a;
    static_cast<StencilArgs&>(a) = stencil_args(*h, b);
    a.aligned = is_aligned(d_src, src_pitch, 16) ? kF32SrcVec : 0;
    a.dst_aligned = is_aligned(d_dst, dst_pitch, 16);
    a.scale = h->scale;
    return launch_bilateral_f32c(h->radius, channels, h->numerics == VIP_NUMERICS_CUDA, a, (hipStream_t)stream);
}

int vip_bilateral_f32_run_c(vip_bilateral_f32_t h, const float* d_src, size_t src_pitch, int channels, float* d_dst,
                            size_t dst_pitch, void* stream) {
    if (!h) return VIP_ERR_INVALID_ARGUMENT;
    return vip_bilateral_f32_run_rows_c(h, d_src, src_pitch, channels, d_dst, dst_pitch, h->height, 0, 0, h->height,
                                        stream);
}

// ---- the f32 bilateral under a second f32 one-channel image, the guide (vip_bilateral_f32j.hpp):
// the same handle, tables and band; the 16-byte accesses are decided for src, guide and dst each on
// its own. d_guide == d_src gives the self-guided result through this filter's own kernel.
constexpr int kMaxKsizeBilateralF32Joint = 2 * kMaxRadius + 1;

int vip_bilateral_f32_max_ksize_joint(void) { return kMaxKsizeBilateralF32Joint; }

int vip_bilateral_f32_run_rows_joint(vip_bilateral_f32_t h, const float* d_src, size_t src_pitch,
                                     const float* d_guide, size_t guide_pitch, float* d_dst, size_t dst_pitch,
                                     int out_rows, int src_row0, int row_lo, int row_hi, void* stream) {
    if (!h || !d_guide) return VIP_ERR_INVALID_ARGUMENT;
    const RowBand b{reinterpret_cast<const uint8_t*>(d_src), src_pitch, reinterpret_cast<const uint8_t*>(d_guide),
                    guide_pitch, reinterpret_cast<uint8_t*>(d_dst), dst_pitch, out_rows, src_row0, row_lo, row_hi};
    if (const int rc = check_band(h->height, b)) return rc;
    if (!is_aligned(d_src, src_pitch, 4) || !is_aligned(d_guide, guide_pitch, 4) || !is_aligned(d_dst, dst_pitch, 4))
        return VIP_ERR_INVALID_ARGUMENT;
    const size_t frow = sizeof(float) * (size_t)h->width;
    if (src_pitch < frow || guide_pitch < frow || dst_pitch < frow) return VIP_ERR_INVALID_ARGUMENT;
    if (h->ksize > kMaxKsizeBilateralF32Joint) return VIP_ERR_UNSUPPORTED_KSIZE;
    BilateralF32Args a;
    static_cast<StencilArgs&>(a) = stencil_args(*h, b);
    a.aligned = (is_aligned(d_src, src_pitch, 16) ? kF32SrcVec : 0) | (is_aligned(d_guide, guide_pitch, 16) ? kF32GuideVec : 0);
    a.dst_aligned = is_aligned(d_dst, dst_pitch, 16);
    a.scale = h->scale;
    return launch_bilateral_f32_joint(h->radius, h->numerics == VIP_NUMERICS_CUDA, a, (hipStream_t)stream);
}

int vip_bilateral_f32_run_joint(vip_bilateral_f32_t h, const float* d_src, size_t src_pitch, const float* d_guide,
                                size_t guide_pitch, float* d_dst, size_t dst_pitch, void* stream) {
    if (!h) return VIP_ERR_INVALID_ARGUMENT;
    return vip_bilateral_f32_run_rows_joint(h, d_src, src_pitch, d_guide, guide_pitch, d_dst, dst_pitch, h->height, 0,
                                            0, h->height, stream);
}

// ---- joint bilateral upsampling (vip_upsample.hip): a handle of its own, since the spatial
// table depends on the scale
static bool valid_scale(int s) { return s == 2 || s == 4 || s == 8; }

// The device table of spatial weights: [n][n], n = scale * radius + scale / 2; entry [ay][ax] is
// the weight of the offset (2 ax + 1, 2 ay + 1) in half full-resolution pixels under
// 2 * scale * sigma_space. Every tap of every phase reads one: its offset
// 2 s k + (s - 1) - 2 p is odd with |.| <= 2 s R + s - 1 = 2 n - 1, and the weight is even in both.
static int upload_upsample_space(vip_upsample_s* h, float sigma_space) {
    const int n = h->scale * h->radius + h->scale / 2;
    const float sigma = (float)(2 * h->scale) * sigma_space;  // exact: a power of two times a float
    std::vector<float> host((size_t)n * n);
    for (int ay = 0; ay < n; ++ay)
        for (int ax = 0; ax < n; ++ax) {
            const int ox = 2 * ax + 1, oy = 2 * ay + 1;
            host[(size_t)ay * n + ax] = space_weight(ox * ox + oy * oy, sigma, h->numerics);
        }
    VIP_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&h->d_wsp), sizeof(float) * host.size()));
    VIP_HIP_CHECK(hipMemcpy(h->d_wsp, host.data(), sizeof(float) * host.size(), hipMemcpyHostToDevice));
    return 0;
}

int vip_upsample_low_size(int width, int height, int scale, int* low_width, int* low_height) {
    if (width <= 0 || height <= 0 || !valid_scale(scale) || !low_width || !low_height) return VIP_ERR_INVALID_ARGUMENT;
    *low_width = (width + scale - 1) / scale;
    *low_height = (height + scale - 1) / scale;
    return 0;
}

int vip_upsample_destroy(vip_upsample_t h) {
    if (!h) return 0;
    if (h->d_wsp) (void)hipFree(h->d_wsp);
    const int rc = h->d_color ? (int)hipFree(h->d_color) : 0;
    delete h;
    return rc;
}

int vip_upsample_create(vip_upsample_t* out, int width, int height, int scale, int ksize, float sigma_space,
                        float sigma_color, int numerics) {
    if (!out || width <= 0 || height <= 0 || !valid_scale(scale)) return VIP_ERR_INVALID_ARGUMENT;
    if (!valid_ksize(ksize, kMaxKsizeUpsample)) return VIP_ERR_UNSUPPORTED_KSIZE;
    vip_upsample_s* h = new (std::nothrow) vip_upsample_s();
    if (!h) return (int)hipErrorOutOfMemory;
    h->width = width;
    h->height = height;
    h->scale = scale;
    h->radius = ksize / 2;
    h->numerics = numerics == VIP_NUMERICS_CPP ? VIP_NUMERICS_CPP : VIP_NUMERICS_CUDA;
    (void)vip_upsample_low_size(width, height, scale, &h->low_width, &h->low_height);
    int nonzero = 0;
    int rc = upload_color(&h->d_color, 768, sigma_color, h->numerics, &nonzero);
    if (!rc) rc = upload_upsample_space(h, sigma_space);
    if (rc) {
        vip_upsample_destroy(h);
        return rc;
    }
    *out = h;
    return 0;
}

// The checks and the kernel arguments of the two upsample entry points: a low-resolution cell and
// an output pixel are `channels` floats; the 16-byte accesses are decided for src and dst each on
// its own
static int upsample_args(vip_upsample_t h, const float* d_src_lo, size_t src_pitch, int channels,
                         const uint8_t* d_guide_lo, size_t guide_lo_pitch, const uint8_t* d_guide, size_t guide_pitch,
                         int guide_channels, float* d_dst, size_t dst_pitch, UpsampleArgs& a) {
    if (!h || !d_src_lo || !d_guide_lo || !d_guide || !d_dst) return VIP_ERR_INVALID_ARGUMENT;
    if (guide_channels != 1 && guide_channels != 3) return VIP_ERR_INVALID_ARGUMENT;
    if (!is_aligned(d_src_lo, src_pitch, 4) || !is_aligned(d_dst, dst_pitch, 4)) return VIP_ERR_INVALID_ARGUMENT;
    const size_t gch = (size_t)guide_channels, cell = sizeof(float) * (size_t)channels;
    if (src_pitch < cell * h->low_width || guide_lo_pitch < gch * h->low_width || guide_pitch < gch * h->width ||
        dst_pitch < cell * h->width)
        return VIP_ERR_INVALID_ARGUMENT;
    const void* const dst = d_dst;
    if (dst == d_src_lo || dst == d_guide_lo || dst == d_guide) return VIP_ERR_ALIASING;
    a = UpsampleArgs{};
    a.src = reinterpret_cast<const uint8_t*>(d_src_lo);
    a.guide_lo = d_guide_lo;
    a.guide = d_guide;
    a.dst = reinterpret_cast<uint8_t*>(d_dst);
    a.src_pitch = (long long)src_pitch;
    a.guide_lo_pitch = (long long)guide_lo_pitch;
    a.guide_pitch = (long long)guide_pitch;
    a.dst_pitch = (long long)dst_pitch;
    a.width = h->width;
    a.out_rows = h->height;
    a.low_width = h->low_width;
    a.low_height = h->low_height;
    a.aligned = (is_aligned(d_guide_lo, guide_lo_pitch, 4) ? kF32GuideWords : 0) |
                (is_aligned(d_src_lo, src_pitch, 16) ? kF32SrcVec : 0) |
                (is_aligned(d_guide, guide_pitch, 4) ? kUpGuideWords : 0);
    a.dst_aligned = is_aligned(d_dst, dst_pitch, 16);
    a.color = h->d_color;
    a.wsp = h->d_wsp;
    return 0;
}

int vip_upsample_run_f32(vip_upsample_t h, const float* d_src_lo, size_t src_pitch, const uint8_t* d_guide_lo,
                         size_t guide_lo_pitch, const uint8_t* d_guide, size_t guide_pitch, int guide_channels,
                         float* d_dst, size_t dst_pitch, void* stream) {
    UpsampleArgs a;
    if (const int rc = upsample_args(h, d_src_lo, src_pitch, 1, d_guide_lo, guide_lo_pitch, d_guide, guide_pitch,
                                     guide_channels, d_dst, dst_pitch, a))
        return rc;
    return launch_upsample_f32(h->radius, h->scale, guide_channels, h->numerics == VIP_NUMERICS_CUDA, a,
                               (hipStream_t)stream);
}

// ---- upsampling of an interleaved field of 2..4 channels (vip_upsample_f32c.hpp), on the same handle
int vip_upsample_run_f32c(vip_upsample_t h, const float* d_src_lo, size_t src_pitch, int channels,
                          const uint8_t* d_guide_lo, size_t guide_lo_pitch, const uint8_t* d_guide,
                          size_t guide_pitch, int guide_channels, float* d_dst, size_t dst_pitch, void* stream) {
    if (channels < 1 || channels > 4) return VIP_ERR_INVALID_ARGUMENT;
    if (channels == 1)
        return vip_upsample_run_f32(h, d_src_lo, src_pitch, d_guide_lo, guide_lo_pitch, d_guide, guide_pitch,
                                    guide_channels, d_dst, dst_pitch, stream);
    UpsampleArgs a;
    if (const int rc = upsample_args(h, d_src_lo, src_pitch, channels, d_guide_lo, guide_lo_pitch, d_guide,
                                     guide_pitch, guide_channels, d_dst, dst_pitch, a))
        return rc;
    return launch_upsample_f32c(h->radius, h->scale, channels, guide_channels, h->numerics == VIP_NUMERICS_CUDA, a,
                                (hipStream_t)stream);
}

// The frames of a *_run_rows_batch call, or a run of them
struct Batch {
    int n;
    const uint8_t* const* srcs;
    uint8_t* const* dsts;
};

// Frames t (t.n <= kMaxBatchFrames) in one StencilArgs built for frame 0: every frame's
// pointers in fsrc/fdst; dword tile loads / qword stores only when every frame allows them.
static void fill_batch(StencilArgs& a, const Batch& t, const RowBand& b) {
    a.nframes = t.n;
    for (int f = 0; f < kMaxBatchFrames; ++f) {
        a.fsrc[f] = t.srcs[f < t.n ? f : 0];
        a.fdst[f] = t.dsts[f < t.n ? f : 0];
        a.aligned = a.aligned && is_aligned(a.fsrc[f], b.src_pitch, 4);
        a.dst_aligned = a.dst_aligned && is_aligned(a.fdst[f], b.dst_pitch, kStencilDstAlign);
    }
}

// Batch arguments: every pointer set, no output that is also an input of the batch.
static int check_batch(const Batch& t) {
    if (t.n < 0 || (t.n > 0 && (!t.srcs || !t.dsts))) return VIP_ERR_INVALID_ARGUMENT;
    for (int f = 0; f < t.n; ++f)
        if (!t.srcs[f] || !t.dsts[f]) return VIP_ERR_INVALID_ARGUMENT;
    for (int f = 0; f < t.n; ++f)
        for (int g = 0; g < t.n; ++g)
            if (t.dsts[f] == t.srcs[g]) return VIP_ERR_ALIASING;
    return 0;
}

// The two *_run_rows_batch entry points (filter: VIP_FILTER_BILATERAL or _ADAPTIVE; only the
// plain bilateral tiling looks at the frames in flight). `b`: the common band, pointers unset.
static int run_batch(const StencilHandle& h, int filter, const Batch& t, RowBand b, int free_cus, hipStream_t s) {
    if (!rows_ok(h.height, b.out_rows, b.row_lo, b.row_hi) || free_cus < 0) return VIP_ERR_INVALID_ARGUMENT;
    if (const int rc = check_batch(t)) return rc;
    if (use_runtime_kernel(h.radius) || h.radius > kBatchMaxRadius) {  // no multi-frame form: frame by frame
        for (int f = 0; f < t.n; ++f) {
            b.src = t.srcs[f];
            b.dst = t.dsts[f];
            if (const int rc = run_band(h, filter, b, nullptr, s)) return rc;
        }
        return 0;
    }
    for (int f0 = 0; f0 < t.n; f0 += kMaxBatchFrames) {
        const Batch run{t.n - f0 < kMaxBatchFrames ? t.n - f0 : kMaxBatchFrames, t.srcs + f0, t.dsts + f0};
        b.src = run.srcs[0];
        b.dst = run.dsts[0];
        StencilArgs a = stencil_args(h, b);
        fill_batch(a, run, b);
        if (filter == VIP_FILTER_BILATERAL) a.inflight = frames_in_flight(s);
        a.free_cus = free_cus;
        if (const int rc = launch_stencil(filter, h.radius, h.numerics == VIP_NUMERICS_CUDA, a, s)) return rc;
    }
    return 0;
}

int vip_bilateral_run_rows_batch(vip_bilateral_t h, int n, const uint8_t* const* d_srcs, size_t src_pitch,
                                 uint8_t* const* d_dsts, size_t dst_pitch, int out_rows, int src_row0, int row_lo,
                                 int row_hi, int free_cus, void* stream) {
    if (!h) return VIP_ERR_INVALID_ARGUMENT;
    const RowBand b{nullptr, src_pitch, nullptr, 0, nullptr, dst_pitch, out_rows, src_row0, row_lo, row_hi};
    return run_batch(*h, VIP_FILTER_BILATERAL, {n, d_srcs, d_dsts}, b, free_cus, (hipStream_t)stream);
}

int vip_bilateral_run(vip_bilateral_t h, const uint8_t* d_src, size_t src_pitch, uint8_t* d_dst, size_t dst_pitch,
                      void* stream) {
    if (!h) return VIP_ERR_INVALID_ARGUMENT;
    return vip_bilateral_run_rows(h, d_src, src_pitch, nullptr, 0, d_dst, dst_pitch, h->height, 0, 0, h->height,
                                  stream);
}

int vip_joint_bilateral_run(vip_bilateral_t h, const uint8_t* d_src, size_t src_pitch, const uint8_t* d_guide,
                            size_t guide_pitch, uint8_t* d_dst, size_t dst_pitch, void* stream) {
    if (!h || !d_guide) return VIP_ERR_INVALID_ARGUMENT;
    return vip_bilateral_run_rows(h, d_src, src_pitch, d_guide, guide_pitch, d_dst, dst_pitch, h->height, 0, 0,
                                  h->height, stream);
}

// ---------------------------------------------------------------- adaptive
int vip_adaptive_create(vip_adaptive_t* out, int width, int height, int ksize, float sigma_space, float sigma_color,
                        int numerics) {
    // the reference's table is 512*3 long (src/adaptive_bilateral_filter_impl.cu:5)
    return create_stencil(out, {width, height, ksize, sigma_space, sigma_color, numerics}, kMaxKsizeAdaptive, 1536);
}

int vip_adaptive_destroy(vip_adaptive_t h) { return destroy_stencil(h); }

int vip_adaptive_run_rows(vip_adaptive_t h, const uint8_t* d_src, size_t src_pitch, uint8_t* d_dst, size_t dst_pitch,
                          int out_rows, int src_row0, int row_lo, int row_hi, void* stream) {
    if (!h) return VIP_ERR_INVALID_ARGUMENT;
    const RowBand b{d_src, src_pitch, nullptr, 0, d_dst, dst_pitch, out_rows, src_row0, row_lo, row_hi};
    if (const int rc = check_band(h->height, b)) return rc;
    return run_band(*h, VIP_FILTER_ADAPTIVE, b, nullptr, (hipStream_t)stream);
}

int vip_adaptive_run_rows_batch(vip_adaptive_t h, int n, const uint8_t* const* d_srcs, size_t src_pitch,
                                uint8_t* const* d_dsts, size_t dst_pitch, int out_rows, int src_row0, int row_lo,
                                int row_hi, int free_cus, void* stream) {
    if (!h) return VIP_ERR_INVALID_ARGUMENT;
    const RowBand b{nullptr, src_pitch, nullptr, 0, nullptr, dst_pitch, out_rows, src_row0, row_lo, row_hi};
    return run_batch(*h, VIP_FILTER_ADAPTIVE, {n, d_srcs, d_dsts}, b, free_cus, (hipStream_t)stream);
}

int vip_adaptive_run(vip_adaptive_t h, const uint8_t* d_src, size_t src_pitch, uint8_t* d_dst, size_t dst_pitch,
                     void* stream) {
    if (!h) return VIP_ERR_INVALID_ARGUMENT;
    return vip_adaptive_run_rows(h, d_src, src_pitch, d_dst, dst_pitch, h->height, 0, 0, h->height, stream);
}

// ---- single-channel form (vip_gray_adaptive.hip): the same band, handle and tables
int vip_adaptive_run_rows_c1(vip_adaptive_t h, const uint8_t* d_src, size_t src_pitch, uint8_t* d_dst,
                             size_t dst_pitch, int out_rows, int src_row0, int row_lo, int row_hi, void* stream) {
    if (!h) return VIP_ERR_INVALID_ARGUMENT;
    const RowBand b{d_src, src_pitch, nullptr, 0, d_dst, dst_pitch, out_rows, src_row0, row_lo, row_hi};
    if (const int rc = check_band(h->height, b)) return rc;
    const bool fma = h->numerics == VIP_NUMERICS_CUDA;
    if (use_runtime_kernel(h->radius)) return launch_gray_adaptive_rt(rt_args(*h, b), fma, (hipStream_t)stream);
    return launch_gray_adaptive(h->radius, fma, stencil_args(*h, b), (hipStream_t)stream);
}

int vip_adaptive_run_c1(vip_adaptive_t h, const uint8_t* d_src, size_t src_pitch, uint8_t* d_dst, size_t dst_pitch,
                        void* stream) {
    if (!h) return VIP_ERR_INVALID_ARGUMENT;
    return vip_adaptive_run_rows_c1(h, d_src, src_pitch, d_dst, dst_pitch, h->height, 0, 0, h->height, stream);
}

// ---------------------------------------------------------------- gradient
int vip_gradient_u8(const uint8_t* d_src, float* d_dst, int width, int height, int src_ch, int numerics,
                    void* stream) {
    (void)numerics;  // u8 arithmetic is exact in both profiles
    if (!d_src || !d_dst || width <= 0 || height <= 0) return VIP_ERR_INVALID_ARGUMENT;
    return launch_gradient_u8(d_src, d_dst, width, height, src_ch, (hipStream_t)stream);
}

int vip_gradient_f32(const float* d_src, float* d_dst, int width, int height, int src_ch, int numerics,
                     void* stream) {
    if (!d_src || !d_dst || width <= 0 || height <= 0) return VIP_ERR_INVALID_ARGUMENT;
    return launch_gradient_f32(d_src, d_dst, width, height, src_ch, numerics != VIP_NUMERICS_CPP,
                               (hipStream_t)stream);
}

// ---------------------------------------------------------------- texture
int vip_texture_destroy(vip_texture_t h) {
    if (!h) return 0;
    vip_bilateral_destroy(h->jbf);
    (void)hipFree(h->d_ping[0]);
    (void)hipFree(h->d_ping[1]);
    (void)hipFree(h->d_guide);
    (void)hipFree(h->d_color_c1);
    delete h;
    return 0;
}

static int upload_color_c1(vip_texture_t h) {
    float wc[768], c1[256];
    build_color(768, 1.73205080757f, h->numerics, wc);
    for (int d = 0; d < 256; ++d) c1[d] = wc[3 * d];
    int nz = 256;
    while (nz > 0 && c1[nz - 1] == 0.f) --nz;
    h->lut_nonzero_c1 = nz;
    VIP_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&h->d_color_c1), sizeof(c1)));
    VIP_HIP_CHECK(hipMemcpy(h->d_color_c1, c1, sizeof(c1), hipMemcpyHostToDevice));
    return 0;
}

int vip_texture_create(vip_texture_t* out, int width, int height, int ksize, int nitr, int numerics) {
    if (!out || width <= 0 || height <= 0 || nitr < 0) return VIP_ERR_INVALID_ARGUMENT;
    // any ksize 1..24 (even too); the embedded JBF has ksize 2k-1 <= 47
    // (src/bilateral_texture_filter_impl.cu:188)
    if (ksize < 1 || ksize > kMaxKsizeTexture) return VIP_ERR_UNSUPPORTED_KSIZE;
    auto* h = new (std::nothrow) vip_texture_s();
    if (!h) return (int)hipErrorOutOfMemory;
    h->width = width;
    h->height = height;
    h->ksize = ksize;
    h->nitr = nitr;
    h->numerics = numerics == VIP_NUMERICS_CPP ? VIP_NUMERICS_CPP : VIP_NUMERICS_CUDA;
    const size_t frame = vip_texture_scratch_bytes(width, height) / 3;
    int rc = vip_bilateral_create(&h->jbf, width, height, 2 * ksize - 1, (float)(ksize - 1), 1.73205080757f,
                                  h->numerics);
    if (!rc) rc = (int)hipMalloc(reinterpret_cast<void**>(&h->d_ping[0]), frame);
    if (!rc) rc = (int)hipMalloc(reinterpret_cast<void**>(&h->d_ping[1]), frame);
    if (!rc) rc = (int)hipMalloc(reinterpret_cast<void**>(&h->d_guide), frame);
    if (!rc) rc = upload_color_c1(h);
    if (rc) {
        vip_texture_destroy(h);
        return rc;
    }
    *out = h;
    return 0;
}

size_t vip_texture_scratch_bytes(int width, int height) {
    if (width <= 0 || height <= 0) return 0;
    return 3 * ((size_t)width * height * 3);  // two ping-pong frames + the guide, u8x3 each
}

int vip_texture_set_mode(vip_texture_t h, int mode) {
    if (!h || (mode != VIP_TEXTURE_TWO_LAUNCH && mode != VIP_TEXTURE_FUSED)) return VIP_ERR_INVALID_ARGUMENT;
    if (mode == VIP_TEXTURE_FUSED && h->ksize != 5) return VIP_ERR_UNSUPPORTED_KSIZE;
    h->mode = mode;
    return 0;
}

int vip_texture_blur_rtv(vip_texture_t h, const uint8_t* d_image, const float* d_magnitude, float* d_blurred,
                         float* d_rtv, void* stream) {
    if (!h || !d_image || !d_magnitude || !d_blurred || !d_rtv) return VIP_ERR_INVALID_ARGUMENT;
    return launch_blur_rtv(d_image, d_magnitude, d_blurred, d_rtv, h->width, h->height, h->ksize,
                           h->numerics == VIP_NUMERICS_CPP, (hipStream_t)stream);
}

int vip_texture_guide(vip_texture_t h, const float* d_blurred, const float* d_rtv, uint8_t* d_guide, void* stream) {
    if (!h || !d_blurred || !d_rtv || !d_guide) return VIP_ERR_INVALID_ARGUMENT;
    return launch_guide(d_blurred, d_rtv, d_guide, h->width, h->height, h->ksize, h->numerics == VIP_NUMERICS_CPP,
                        (hipStream_t)stream);
}

static int texture_run(vip_texture_t h, const uint8_t* d_src, uint8_t* d_dst, void* stream, void* const* events) {
    if (!h || !d_src || !d_dst) return VIP_ERR_INVALID_ARGUMENT;
    const hipStream_t s = (hipStream_t)stream;
    const size_t bytes = (size_t)h->width * h->height * 3;
    const size_t pitch = (size_t)h->width * 3;
    if (h->nitr == 0) {
        if (events) VIP_HIP_CHECK(hipEventRecord((hipEvent_t)events[0], s));
        if (d_src != d_dst) VIP_HIP_CHECK(hipMemcpyAsync(d_dst, d_src, bytes, hipMemcpyDeviceToDevice, s));
        return 0;
    }
    const uint8_t* cur = d_src;
    if (d_src == d_dst) {  // the last JBF must not write the frame it reads
        VIP_HIP_CHECK(hipMemcpyAsync(h->d_ping[1], d_src, bytes, hipMemcpyDeviceToDevice, s));
        cur = h->d_ping[1];
    }
    for (int it = 0; it < h->nitr; ++it) {
        uint8_t* next = (it == h->nitr - 1) ? d_dst : (cur == h->d_ping[0] ? h->d_ping[1] : h->d_ping[0]);
        // gradient -> blur/mRTV -> guide fused in LDS (one launch), then the JBF
        if (events) VIP_HIP_CHECK(hipEventRecord((hipEvent_t)events[2 * it], s));
        int rc;
        if (h->mode == VIP_TEXTURE_FUSED) {  // guide + JBF in one launch, the guide stays in LDS
            const RowBand b{cur, pitch, nullptr, 0, next, pitch, h->height, 0, 0, h->height};
            rc = launch_texture_iteration_fused(stencil_args(*h->jbf, b), h->ksize, h->numerics == VIP_NUMERICS_CPP,
                                                s);
            if (!rc && events) rc = (int)hipEventRecord((hipEvent_t)events[2 * it + 1], s);
        } else {
            rc = launch_texture_guide_fused(cur, h->d_guide, h->width, h->height, h->ksize,
                                            h->numerics == VIP_NUMERICS_CPP, s);
            if (!rc && events) rc = (int)hipEventRecord((hipEvent_t)events[2 * it + 1], s);
            if (!rc) rc = vip_joint_bilateral_run(h->jbf, cur, pitch, h->d_guide, pitch, next, pitch, stream);
        }
        if (rc) return rc;
        cur = next;
    }
    if (events) VIP_HIP_CHECK(hipEventRecord((hipEvent_t)events[2 * h->nitr], s));
    return 0;
}

// Impl::execute (src/bilateral_texture_filter_impl.cu:199-214) without the
// nitr + 2 device-to-device copies: iteration i reads X_i and writes X_{i+1},
// X_0 = d_src, X_nitr = d_dst, intermediates alternate between two scratch frames.
// Each iteration is two launches: the fused guide stage and the joint bilateral.
int vip_texture_run(vip_texture_t h, const uint8_t* d_src, uint8_t* d_dst, void* stream) {
    return texture_run(h, d_src, d_dst, stream, nullptr);
}

int vip_texture_run_timed(vip_texture_t h, const uint8_t* d_src, uint8_t* d_dst, void* stream, void* const* events) {
    if (!events) return VIP_ERR_INVALID_ARGUMENT;
    return texture_run(h, d_src, d_dst, stream, events);
}

// The one-channel filter (vip.h): per iteration the one-channel guide stage
// (vip_gray_texture.hip) and the gray joint bilateral under that gray guide (vip_gray.hip),
// with the handle's 256-entry table. Gray frames in the handle's u8x3 scratch frames: rows
// of gray_pitch bytes (dword-aligned rows from width 4 on; never more than a third of a frame).
static size_t gray_pitch(int width) { return width < 4 ? (size_t)width : (size_t)round_up(width, 4); }

int vip_texture_run_c1(vip_texture_t h, const uint8_t* d_src, size_t src_pitch, uint8_t* d_dst, size_t dst_pitch,
                       void* stream) {
    if (!h || !d_src || !d_dst || src_pitch < (size_t)h->width || dst_pitch < (size_t)h->width)
        return VIP_ERR_INVALID_ARGUMENT;
    const hipStream_t s = (hipStream_t)stream;
    const size_t gp = gray_pitch(h->width);
    if (h->nitr == 0) {
        if (d_src != d_dst)
            VIP_HIP_CHECK(hipMemcpy2DAsync(d_dst, dst_pitch, d_src, src_pitch, (size_t)h->width, (size_t)h->height,
                                           hipMemcpyDeviceToDevice, s));
        return 0;
    }
    const uint8_t* cur = d_src;
    size_t cur_pitch = src_pitch;
    if (d_src == d_dst) {  // the last JBF must not write the frame it reads
        VIP_HIP_CHECK(hipMemcpy2DAsync(h->d_ping[1], gp, d_src, src_pitch, (size_t)h->width, (size_t)h->height,
                                       hipMemcpyDeviceToDevice, s));
        cur = h->d_ping[1];
        cur_pitch = gp;
    }
    StencilHandle jbf = *h->jbf;  // the JBF's geometry and spatial tables, the gray guide's colour table
    jbf.d_color = h->d_color_c1;
    jbf.lut_nonzero = h->lut_nonzero_c1;
    const bool fma = h->numerics == VIP_NUMERICS_CUDA;
    for (int it = 0; it < h->nitr; ++it) {
        const bool last = it == h->nitr - 1;
        uint8_t* next = last ? d_dst : (cur == h->d_ping[0] ? h->d_ping[1] : h->d_ping[0]);
        const size_t next_pitch = last ? dst_pitch : gp;
        int rc = launch_gray_texture_guide_rows(cur, cur_pitch, h->d_guide, gp, h->width, 0, h->height, 0, h->height,
                                                h->ksize, !fma, s);
        if (rc) return rc;
        const RowBand b{cur, cur_pitch, h->d_guide, gp, next, next_pitch, h->height, 0, 0, h->height};
        rc = use_runtime_kernel(jbf.radius) ? launch_gray_rt(rt_args(jbf, b), 1, fma, s)
                                            : launch_gray(jbf.radius, 1, fma, stencil_args(jbf, b), s);
        if (rc) return rc;
        cur = next;
        cur_pitch = next_pitch;
    }
    return 0;
}

int vip_texture_halo_rows(int ksize) {
    if (ksize < 1) return VIP_ERR_INVALID_ARGUMENT;
    // JBF radius (2k-1)/2 = k-1 on the guide, whose stages reach gradient 1 + blur/mRTV
    // k/2 + argmin k/2 rows further into the image
    return (ksize - 1) + 2 * (ksize / 2) + 1;
}

// One iteration on a row slab (multi-GPU texture filter): guide rows
// [out_row0 - (k-1), out_row0 + out_rows + (k-1)) clipped to the valid rows, then
// the JBF of the output rows. Stage reads clamp into [row_lo, row_hi), so at a
// frame edge the result is the reference's; elsewhere the caller supplies
// vip_texture_halo_rows(k) valid rows around the output rows.
int vip_texture_iterate_rows(vip_texture_t h, const uint8_t* d_src, uint8_t* d_dst, size_t dst_pitch, int out_row0,
                             int out_rows, int row_lo, int row_hi, void* stream) {
    if (!h || !d_src || !d_dst || !rows_ok(h->height, out_rows, row_lo, row_hi) || out_row0 < row_lo ||
        out_row0 + out_rows > row_hi)
        return VIP_ERR_INVALID_ARGUMENT;
    if (out_rows == 0) return 0;
    const size_t pitch = (size_t)h->width * 3;
    const uint8_t* dst_end = d_dst + (size_t)(out_rows - 1) * dst_pitch + pitch;
    const uint8_t* src_end = d_src + (size_t)h->height * pitch;
    if (d_dst < src_end && dst_end > d_src) return VIP_ERR_ALIASING;
    const int rj = h->ksize - 1;
    const int g0 = out_row0 - rj > row_lo ? out_row0 - rj : row_lo;
    const int g1 = out_row0 + out_rows + rj < row_hi ? out_row0 + out_rows + rj : row_hi;
    const hipStream_t s = (hipStream_t)stream;
    int rc = launch_texture_guide_fused_rows(d_src, h->d_guide, h->width, row_lo, row_hi, g0, g1, h->ksize,
                                             h->numerics == VIP_NUMERICS_CPP, s);
    if (!rc) rc = vip_bilateral_run_rows(h->jbf, d_src, pitch, h->d_guide, pitch, d_dst, dst_pitch, out_rows,
                                         out_row0, row_lo, row_hi, stream);
    return rc;
}

}  // extern "C"
