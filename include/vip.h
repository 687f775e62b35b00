/*
 * vip.h — C ABI of the MI355X-native bilateral-filter family.
 *
 * Drop-in boundary for the reference's include/cuda/ headers' API
 * (yuyuyu-bot/various_image_processings). Plain pointers and sizes only; every
 * image pointer is a DEVICE pointer to dense interleaved 8-bit 3-channel data
 * (or f32 where stated; the *_c1 entry points take 8-bit 1-channel images).
 * `pitch` arguments are row strides in bytes; the
 * reference API has no pitch, so its wrappers pass width*channels*sizeof(T).
 * `stream` is a hipStream_t (NULL = the legacy default stream). Every run
 * function is asynchronous on `stream`: the C++ wrappers in include/cuda/ add
 * the device synchronisation the reference performs in its public methods.
 *
 * Return value: 0 on success, otherwise a hipError_t code, or one of the
 * VIP_ERR_* codes below for argument errors (the reference printed launch errors
 * to stderr and carried on, src/host_utilities.hpp:9-13).
 */
#ifndef VIP_H
#define VIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VIP_ABI_VERSION 1

/* numerics profile */
#define VIP_NUMERICS_CUDA 0 /* as src/<filter>_impl.cu: float-coefficient LUTs, fused multiply-add accumulate */
#define VIP_NUMERICS_CPP 1  /* as include/cpp/<filter>.hpp: double-coefficient LUTs, separate multiply and add */

/* argument errors (hipError_t values stay below 1000) */
#define VIP_ERR_INVALID_ARGUMENT 10001 /* null handle/pointer, non-positive size */
#define VIP_ERR_UNSUPPORTED_KSIZE 10002 /* ksize outside what the reference runs: see vip_max_ksize */
#define VIP_ERR_ALIASING 10003 /* dst aliases src or guide (the kernels read neighbours other blocks write) */

typedef struct vip_bilateral_s* vip_bilateral_t;
typedef struct vip_adaptive_s* vip_adaptive_t;
typedef struct vip_texture_s* vip_texture_t;
typedef struct vip_upsample_s* vip_upsample_t;

int vip_abi_version(void);
/* The kernels the calling thread launched through this library since its previous call,
 * as the profiler names them ("void vip::bilateral_kernel<7, 16, ...>", no parameter
 * list), newline-separated, each once. With a buffer (len > 0) it writes at most len - 1
 * bytes and a terminating 0 and clears the list; buf = NULL, len = 0 only returns the
 * length. Returns the full length. No reference counterpart: it lets a benchmark
 * name the exact template instantiation it timed. */
int vip_launched_kernels(char* buf, size_t len);
/* Kernel-duration recorder of the calling thread (measurement; no reference counterpart).
 * After vip_kernel_timing_begin(capacity) the next `capacity` kernels this thread launches
 * through the library carry a (start, stop) event pair that the runtime stamps with the
 * kernel's own begin and end (hipExtLaunchKernel): no marker packet enters the stream, so a
 * duration is what rocprofv3 --kernel-trace reports for that launch. Begin clears earlier
 * records (capacity 1..65536). vip_kernel_timing_end() stops recording and returns the
 * number of launches recorded. vip_kernel_timing_get(i, &ms, name, len), after end, waits
 * for launch i to finish and returns its duration and (if name) its kernel name as
 * vip_launched_kernels names it. */
int vip_kernel_timing_begin(int capacity);
int vip_kernel_timing_end(void);
int vip_kernel_timing_get(int index, float* ms, char* name, size_t len);
const char* vip_error_string(int code);
/* Largest filter radius (ksize/2) any filter accepts (32: bilateral ksize 65). */
int vip_max_radius(void);

/* Largest ksize each filter accepts: what the reference runs. Its kernels size dynamic
 * shared memory from ksize with no cap against CUDA's 48 KB default
 * (src/bilateral_filter_impl.cu:252-254, 272-275; src/adaptive_bilateral_filter_impl.cu:165-167),
 * so: bilateral 65, joint bilateral 47, adaptive 63, texture 24 (its JBF is 2k-1 <= 47).
 * Bilateral, joint and adaptive take odd ksize from 1 (radius 0: output = input for
 * sigma_space > 0); the texture filter any ksize from 1. The C++ and Python layers take
 * the same sets. Joint bilateral upsampling (no reference counterpart) takes odd ksize 1..9,
 * in low-resolution pixels; the confidence-weighted f32 joint bilateral (VIP_FILTER_JOINT_CONF) odd
 * ksize 1..31; the f32 joint bilateral on 2..4 interleaved channels (VIP_FILTER_JOINT_F32C) an odd
 * ksize up to a cap that depends on the channel count: vip_max_ksize gives the largest, 31 (two
 * channels), vip_joint_f32c_max_ksize(channels) each: 1: 47 (the f32 joint filter itself), 2: 31,
 * 3: 15, 4: 15, VIP_ERR_INVALID_ARGUMENT otherwise.
 * Returns VIP_ERR_INVALID_ARGUMENT for an unknown filter. */
#define VIP_FILTER_BILATERAL 0
#define VIP_FILTER_JOINT 1
#define VIP_FILTER_ADAPTIVE 2
#define VIP_FILTER_TEXTURE 3
#define VIP_FILTER_UPSAMPLE 4
#define VIP_FILTER_JOINT_CONF 5
#define VIP_FILTER_JOINT_F32C 6
int vip_max_ksize(int filter);
int vip_joint_f32c_max_ksize(int channels);

/* Kernel selection, process-wide (no reference counterpart; results are identical either
 * way). AUTO: radius-specialised kernels for radius 1..15, the runtime-radius kernel for
 * radius 0 and 16..32. RUNTIME: the runtime-radius kernel for every radius (test and
 * measurement knob). The environment variable VIP_STENCIL_PATH=1 sets RUNTIME at load. */
#define VIP_PATH_AUTO 0
#define VIP_PATH_RUNTIME 1
int vip_set_stencil_path(int path);

/* ---- device buffers: replaces DeviceImage<T> (include/cuda/device_image.hpp:4-16,
 *      src/device_image.cu:5-52) ---- */
int vip_malloc(void** d_ptr, size_t bytes);
int vip_free(void* d_ptr);
int vip_upload(void* d_dst, const void* h_src, size_t bytes);   /* blocking H2D */
int vip_download(void* h_dst, const void* d_src, size_t bytes); /* blocking D2H */
int vip_device_synchronize(void);
int vip_stream_synchronize(void* stream);
/* Device selection for multi-GPU callers (the reference drives the implicit current
 * device only): every handle, buffer and launch belongs to the calling thread's
 * current device at the time of the call. */
int vip_device_count(int* count);
int vip_set_device(int device);
int vip_get_device(int* device);

/* ---- host-frame path (the reference's DeviceImage::upload/download,
 *      src/device_image.cu:10-16, copy pageable memory synchronously through thrust).
 *      Pinned host frames + stream-ordered copies let H2D, kernels and D2H of
 *      successive frames overlap on separate streams. ---- */
int vip_host_alloc(void** h_ptr, size_t bytes);  /* page-locked host memory */
int vip_host_free(void* h_ptr);
int vip_upload_async(void* d_dst, const void* h_src, size_t bytes, void* stream);   /* stream-ordered H2D */
int vip_download_async(void* h_dst, const void* d_src, size_t bytes, void* stream); /* stream-ordered D2H */
int vip_stream_create(void** stream);  /* non-blocking HIP stream, returned as void* */
int vip_stream_destroy(void* stream);
/* Cross-stream ordering for a split pipeline (one upload, one compute and one download
 * stream): H2D and D2H on their own streams overlap (measured 0.52 ms per 4K frame
 * pair vs 0.89 ms when one stream carries both directions). No timing. */
int vip_event_create(void** event);
int vip_event_destroy(void* event);
int vip_event_record(void* event, void* stream);
int vip_stream_wait_event(void* stream, void* event); /* later work on stream waits for event */
int vip_event_synchronize(void* event);               /* host waits for event */

/* ---- bilateral / joint bilateral: CudaBilateralFilter
 *      (include/cuda/bilateral_filter.hpp:9-24, src/bilateral_filter_impl.cu:204-310) ---- */
int vip_bilateral_create(vip_bilateral_t* out, int width, int height, int ksize, float sigma_space,
                         float sigma_color, int numerics);
int vip_bilateral_destroy(vip_bilateral_t h);
/* Impl::bilateral_filter (:241-258) */
int vip_bilateral_run(vip_bilateral_t h, const uint8_t* d_src, size_t src_pitch, uint8_t* d_dst, size_t dst_pitch,
                      void* stream);
/* Impl::joint_bilateral_filter (:260-280): colour weights from d_guide, sums of d_src */
int vip_joint_bilateral_run(vip_bilateral_t h, const uint8_t* d_src, size_t src_pitch, const uint8_t* d_guide,
                            size_t guide_pitch, uint8_t* d_dst, size_t dst_pitch, void* stream);
/* Row-band variant for row-sharded frames (no reference counterpart; multi-GPU C5).
 * Filters `out_rows` rows of a handle-width image. Output row i is centred on source
 * row i + src_row0; neighbour rows are clamped to [row_lo, row_hi) of d_src, with
 * 0 <= row_lo < row_hi <= the handle's height (d_src and d_guide hold that many rows;
 * rows below row_lo / above row_hi-1 replicate them, which is exactly the reference's
 * replicate border at the frame edges). d_guide may be NULL (plain bilateral).
 * Returns VIP_ERR_INVALID_ARGUMENT for a row range outside the handle's rows. */
int vip_bilateral_run_rows(vip_bilateral_t h, const uint8_t* d_src, size_t src_pitch, const uint8_t* d_guide,
                           size_t guide_pitch, uint8_t* d_dst, size_t dst_pitch, int out_rows, int src_row0,
                           int row_lo, int row_hi, void* stream);
/* n frames of the same geometry (no reference counterpart; a shard's frames per RCCL group,
 * vip_shard_run_batch): frame f filters d_srcs[f] into d_dsts[f] exactly as
 * vip_bilateral_run_rows(h, d_srcs[f], src_pitch, NULL, 0, d_dsts[f], dst_pitch, out_rows,
 * src_row0, row_lo, row_hi, stream) would, with up to 6 frames per launch: the persistent
 * workgroups run from one frame's tiles into the next one's, so a small slab's launch
 * prologue and tail are paid once per launch. free_cus >= 0: CUs the launch leaves to
 * concurrent work (another stream's frames, an exchange kernel); 0 = all CUs.
 * VIP_ERR_ALIASING when any d_dsts[f] equals any d_srcs[g]. Results are identical to the
 * per-frame calls. */
int vip_bilateral_run_rows_batch(vip_bilateral_t h, int n, const uint8_t* const* d_srcs, size_t src_pitch,
                                 uint8_t* const* d_dsts, size_t dst_pitch, int out_rows, int src_row0, int row_lo,
                                 int row_hi, int free_cus, void* stream);
/* ---- single-channel (8-bit gray) forms (no reference counterpart). d_src and d_dst are one
 * byte per pixel; the handle is the same vip_bilateral_t, with its spatial LUT and its
 * 768-entry colour LUT. Per tap in row-major order over the k x k square, replicate border:
 *   w = ws[ky,kx] * wc[d];  s += g_n * w (fused in the CUDA profile);  sumk += w;
 *   dst = u8(s / sumk + 0.5f)
 * with d = |g_n - g_c| (plain), |G_n - G_c| (guide_channels 1: a gray guide G; only the
 * first 256 LUT entries are reached) or |dB| + |dG| + |dR| (guide_channels 3: an interleaved
 * 3-channel guide). Each result is, bit for bit, channel 0 of the 3-channel filter on the
 * frame (g, 0, 0) (with the guide (G, 0, 0) for a gray guide), and what OpenCV's 8UC1
 * bilateral weighs by. Plain ksize 1..65 odd, joint 1..47 odd (VIP_ERR_UNSUPPORTED_KSIZE for
 * a joint call on a larger handle). Any base address and pitch work for d_src, d_guide and
 * d_dst: the kernels use dword loads / word stores only where the addresses allow, and
 * never write a byte of d_dst at column >= width or row >= out_rows (row padding stays the
 * caller's). One launch per call, no device allocation, no intermediate 3-channel buffer.
 * VIP_ERR_INVALID_ARGUMENT: null handle or pointer, a bad band, guide_channels not 1 or 3
 * with a guide; VIP_ERR_ALIASING: d_dst equals d_src or d_guide. The gray kernels honour
 * vip_set_stencil_path as the 3-channel ones do (AUTO: radius-specialised vip::gray_kernel
 * for radius 1..15, vip::gray_rt_kernel for 0 and 16..32; RUNTIME: gray_rt_kernel always);
 * vip_bilateral_set_waves / _set_wide / _set_frames_in_flight do not apply to them. */
int vip_bilateral_run_c1(vip_bilateral_t h, const uint8_t* d_src, size_t src_pitch, uint8_t* d_dst, size_t dst_pitch,
                         void* stream);
int vip_joint_bilateral_run_c1(vip_bilateral_t h, const uint8_t* d_src, size_t src_pitch, const uint8_t* d_guide,
                               size_t guide_pitch, int guide_channels, uint8_t* d_dst, size_t dst_pitch,
                               void* stream);
/* Row band, as vip_bilateral_run_rows; d_guide NULL: plain (guide_channels is then ignored) */
int vip_bilateral_run_rows_c1(vip_bilateral_t h, const uint8_t* d_src, size_t src_pitch, const uint8_t* d_guide,
                              size_t guide_pitch, int guide_channels, uint8_t* d_dst, size_t dst_pitch, int out_rows,
                              int src_row0, int row_lo, int row_hi, void* stream);
/* ---- joint bilateral of an f32 one-channel source under an 8-bit guide (no counterpart in the
 * reference's API; OpenCV's ximgproc::jointBilateralFilter takes this pair): a depth, disparity,
 * flow, matte or cost field f smoothed under a gray (guide_channels 1) or interleaved 3-channel
 * (guide_channels 3) 8-bit image G. The handle is the same vip_bilateral_t, radius ksize / 2,
 * with its spatial LUT ws and its 768-entry colour LUT wc; borders replicate. Per output pixel
 * the taps run in row-major order over the k x k square:
 *   d    = |G_n - G_c|            (guide_channels 1; reaches LUT entries 0..255)
 *        = |dB| + |dG| + |dR|     (guide_channels 3; 0..765)
 *   w    = ws[ky,kx] * wc[d]      (ws is exactly 0 outside the disc)
 *   s    = fmaf(f_n, w, s)        VIP_NUMERICS_CUDA
 *   s    = s + f_n * w            VIP_NUMERICS_CPP (two roundings)
 *   sumk = sumk + w
 *   dst  = s / sumk               IEEE binary32 division, no rounding to integer, no clamp
 * Arithmetic is binary32 with gradual underflow: the build's -O3 -ffp-contract=off leaves the
 * kernels in denormal mode 3 (.amdhsa_float_denorm_mode_32 3 in every kernel descriptor).
 * sumk >= 1 always (the centre tap has w = 1).
 * Domain: every source value must be finite. For finite input the result equals the definition
 * bit for bit, in both profiles and on both kernel paths. With an Inf or NaN in the source the
 * values are unspecified (the runtime-radius kernel also multiplies out-of-disc neighbours by an
 * exact zero weight, a no-op only for finite neighbours), but such a call cannot fault:
 * every address comes from the guide. Sums that overflow give +-Inf, as in the definition.
 * Tie to the 8-bit form: for f == (float)g with a gray u8 frame g, u8(dst + 0.5f) is
 * vip_joint_bilateral_run_c1 on g, bit for bit (s and sumk are the same floats).
 * ksize 1..47 odd (VIP_ERR_UNSUPPORTED_KSIZE on a larger handle); ksize 1 returns f, except that
 * -0 becomes +0 (s starts at +0: fmaf(-0, 1, +0) = +0 and (+0) + (-0 * 1) = +0, in both profiles).
 * Pitches are in bytes. d_src and d_dst bases and pitches must be multiples of 4
 * (VIP_ERR_INVALID_ARGUMENT otherwise); any such value works: the kernels take 16-byte loads
 * and stores only where base and pitch are multiples of 16, dword accesses otherwise. d_guide
 * may have any base and pitch. No byte of d_dst at column >= width or row >= out_rows is
 * written. VIP_ERR_INVALID_ARGUMENT: null handle or pointer (a null guide too: there is no
 * plain f32 form), a bad band, guide_channels not 1 or 3; VIP_ERR_ALIASING: d_dst equals d_src
 * or d_guide. One launch per call, no device allocation. Kernels under VIP_PATH_AUTO:
 * vip::joint_f32_kernel<R, GUIDE, FMA> for radius 1..15 (gray guide: 32 LUT copies, 16-wave
 * workgroups and 128 x 64 tiles up to radius 12, 12 waves and 128 x 48 tiles for radius 13..15;
 * 3-channel guide: 16 LUT copies, 16 waves up to radius 9, 12 waves for radius 10..15),
 * vip::joint_f32_rt_kernel<GUIDE, FMA> (64 x 64 tiles, the same LUTs) for radius 0 and
 * 16..23; under VIP_PATH_RUNTIME joint_f32_rt_kernel for every radius. The launch log and
 * vip_kernel_timing_* see them; vip_bilateral_set_waves / _set_wide / _set_frames_in_flight do
 * not apply. The _rows form takes a row band as vip_bilateral_run_rows_c1. */
int vip_joint_bilateral_run_f32(vip_bilateral_t h, const float* d_src, size_t src_pitch, const uint8_t* d_guide,
                                size_t guide_pitch, int guide_channels, float* d_dst, size_t dst_pitch,
                                void* stream);
int vip_joint_bilateral_run_rows_f32(vip_bilateral_t h, const float* d_src, size_t src_pitch,
                                     const uint8_t* d_guide, size_t guide_pitch, int guide_channels, float* d_dst,
                                     size_t dst_pitch, int out_rows, int src_row0, int row_lo, int row_hi,
                                     void* stream);
/* ---- confidence-weighted joint bilateral of an f32 one-channel source (normalised convolution
 * under an image guide; no counterpart in the reference's API): a field f with holes or with a
 * per-pixel confidence c is smoothed under the 8-bit guide G, and pixels without a valid value are
 * filled from the valid ones in reach. With a 0/1 mask as c it is hole filling, with a solver's
 * confidence the usual confidence-weighted refinement. ws, wc, the row-major tap order over the
 * k x k square, the replicate border and d are those of vip_joint_bilateral_run_f32.
 * Per pixel, formed once:
 *   p = (c == 0) ? +0.0f : f * c     one binary32 product; f is not used as a number where c == 0
 * Per output pixel and tap:
 *   w    = ws[ky,kx] * wc[d]
 *   s    = fmaf(p_n, w, s)    sumk = fmaf(c_n, w, sumk)      VIP_NUMERICS_CUDA
 *   s    = s + p_n * w        sumk = sumk + c_n * w          VIP_NUMERICS_CPP (two roundings each)
 *   dst    = (sumk == 0) ? hole_value : s / sumk             IEEE binary32 division
 *   weight = sumk                                            written only if d_weight != NULL
 * Arithmetic is binary32 with gradual underflow (denormal mode 3, as the sibling kernels).
 * Domain: c is finite and >= 0 (-0.0f counts as 0); f is finite wherever c > 0. Where c == 0, f may
 * hold anything, NaN and Inf included: the output is, bit for bit, independent of it. Outside the
 * domain the values are unspecified, but the call cannot fault: every address comes from
 * coordinates and the guide.
 * Ties that hold bit for bit: with c == 1 everywhere dst equals vip_joint_bilateral_run_f32 on f
 * (p = f and fmaf(1, w, sumk) = sumk + w); with c == 2^-2 everywhere dst is the same as with
 * c == 1, on inputs free of underflow.
 * ksize 1..31 odd (vip_max_ksize(VIP_FILTER_JOINT_CONF)); a handle with a larger ksize gives
 * VIP_ERR_UNSUPPORTED_KSIZE. The cap: the filter keeps three LDS planes (guide word, p, c) where
 * the f32 filter keeps two, and three planes under the runtime-radius kernel's 64 x 64 tile stop
 * fitting LDS near radius 12..16, so there is no runtime-radius kernel here; depth and disparity
 * refinement lives at these sizes. ksize 1 gives dst = c == 0 ? hole_value : fl(f * c) / c.
 * vip_set_stencil_path and the vip_bilateral_set_* knobs do not apply.
 * Pitches are in bytes. The float bases and pitches (d_src, d_conf, d_dst, d_weight) must be
 * multiples of 4; 16-byte accesses are used only where base and pitch allow them, decided per
 * array. d_guide may have any base and pitch. No byte of d_dst or d_weight at column >= width or
 * row >= height is written. VIP_ERR_INVALID_ARGUMENT: null handle, d_src, d_conf, d_guide or
 * d_dst; guide_channels not 1 or 3; a misaligned float base or pitch; a pitch smaller than a row.
 * VIP_ERR_ALIASING: d_dst or d_weight equals any input, or the two are equal. One launch per call,
 * no device allocation: vip::joint_conf_f32_kernel<R, GUIDE, FMA> for radius 1..15,
 * vip::joint_conf_f32_k1_kernel<FMA> for ksize 1; the launch log and vip_kernel_timing_* see them.
 * Against today's route (two vip_joint_bilateral_run_f32 launches on f * c and c, two elementwise
 * passes): see DESIGN.md section 4 for the measured times; nothing here promises a speed. */
int vip_joint_bilateral_run_conf_f32(vip_bilateral_t h, const float* d_src, size_t src_pitch, const float* d_conf,
                                     size_t conf_pitch, const uint8_t* d_guide, size_t guide_pitch,
                                     int guide_channels, float hole_value, float* d_dst, size_t dst_pitch,
                                     float* d_weight /* may be NULL */, size_t weight_pitch, void* stream);
/* ---- joint bilateral of an interleaved f32 source of 1..4 channels under an 8-bit guide (no
 * counterpart in the reference's API): optical flow (2 channels), normals or float colour (3),
 * RGBA, premultiplied colour or a small cost slice (4), every channel smoothed under the same
 * guide in one launch. In a joint filter the weights come from the guide alone, so they are
 * formed once per tap and serve every channel.
 * d_src and d_dst are interleaved: channel c of pixel (x, y) is
 *   ((float*)(base + y * pitch))[x * channels + c]
 * The handle, ws, wc, the replicate border, d, the row-major tap order over the k x k square and
 * the two numerics profiles are those of vip_joint_bilateral_run_f32. Per output pixel and tap:
 *   w    = ws[ky,kx] * wc[d]            formed once
 *   s_c  = fmaf(f_c(n), w, s_c)         for each channel c, VIP_NUMERICS_CUDA
 *   s_c  = s_c + f_c(n) * w             for each channel c, VIP_NUMERICS_CPP (two roundings)
 *   sumk = sumk + w                     once
 *   dst_c = s_c / sumk                  IEEE binary32 division, no rounding to integer, no clamp
 * Arithmetic is binary32 with gradual underflow (denormal mode 3, as the sibling kernels).
 * Domain: every source value must be finite.
 * Tie that holds bit for bit: for every c, plane c of dst is what vip_joint_bilateral_run_f32
 * writes for plane c of src, in both profiles and with both guides, signed zeros and subnormals
 * included. With an Inf or NaN in the source the values are unspecified, but the call cannot
 * fault: every address comes from coordinates and the guide.
 * channels 1 forwards to vip_joint_bilateral_run_f32 (the same kernels, the same ksize cap of 47,
 * the same checks), so a caller generic over the channel count needs no branch. channels 2 takes
 * odd ksize 1..31, channels 3 and 4 odd ksize 1..15 (vip_joint_f32c_max_ksize); a handle above
 * the cap gives VIP_ERR_UNSUPPORTED_KSIZE. The caps: the filter keeps channels + 1 LDS planes
 * (guide word, f_0 ..) where the f32 filter keeps two, and there is no runtime-radius kernel for
 * channels >= 2; vip_set_stencil_path and the vip_bilateral_set_* knobs do not apply.
 * Pitches are in bytes. The float bases and pitches must be multiples of 4; 16-byte accesses are
 * used only where base and pitch are multiples of 16, decided separately for d_src and d_dst.
 * d_guide may have any base and pitch. No byte of d_dst is written at a byte offset
 * >= width * channels * 4 within a row, nor at a row >= height.
 * VIP_ERR_INVALID_ARGUMENT: a null handle or pointer; channels outside 1..4; guide_channels not 1
 * or 3; a misaligned float base or pitch; a pitch smaller than a row. VIP_ERR_ALIASING: d_dst
 * equals d_src or d_guide. One launch per call, asynchronous, no device allocation:
 * vip::joint_f32c_kernel<R, C, GUIDE, FMA> for radius 1..15 (C = 2) or 1..7 (C = 3, 4),
 * vip::joint_f32c_k1_kernel<C, FMA> for ksize 1 (dst_c = fmaf(f_c, w, 0) / (0 + w) with
 * w = ws[0] * wc[0]; the guide is not read); the launch log and vip_kernel_timing_* see them.
 * Against C launches of vip_joint_bilateral_run_f32 on de-interleaved planes: see DESIGN.md
 * section 4 for the measured times; nothing here promises a speed. */
int vip_joint_bilateral_run_f32c(vip_bilateral_t h, const float* d_src, size_t src_pitch, int channels,
                                 const uint8_t* d_guide, size_t guide_pitch, int guide_channels, float* d_dst,
                                 size_t dst_pitch, void* stream);
/* ---- self-guided bilateral filter of an f32 one-channel image (no counterpart in the reference's
 * API; OpenCV's cv::bilateralFilter takes CV_32F): a depth or disparity map on its own, an HDR
 * luminance plane, a height field, the base layer of a tone-mapper. The float image is its own
 * guide. As OpenCV's 32F path, the range weight is a quantised table with linear interpolation:
 * N = VIP_BILATERAL_F32_BINS bins cover differences 0..value_range, so every operation is a
 * binary32 operation and the range weight costs one table read per tap, not an exp.
 * Tables, built on the host at create time; cf = -1.f / (2 * sigma_color * sigma_color) (float) and
 * cd = -1. / (double)(2 * sigma_color * sigma_color), as the colour LUT of vip_bilateral_create:
 *   scale    = (float)N / value_range                float division
 *   v        = (float)i / scale                      float division, i = 0..N
 *   L[i]     = expf((v * v) * cf)                    VIP_NUMERICS_CUDA: float product, host expf
 *   L[i]     = (float)exp((double)v * (double)v * cd)   VIP_NUMERICS_CPP
 *   L[N + 1] = L[N]
 *   D[i]     = L[i + 1] - L[i]                       float, i = 0..N; D[N] = 0
 *   ws       the spatial table of vip_bilateral_create at radius ksize / 2, exactly 0 outside the disc
 * Per output pixel the taps run in row-major order over the k x k square, replicate border:
 *   d    = |f_n - f_c|                  binary32 subtract, then abs
 *   t    = min(d * scale, (float)N)
 *   i    = (int)t;  a = t - (float)i    (exact)
 *   wc   = fmaf(a, D[i], L[i])          VIP_NUMERICS_CUDA
 *   wc   = L[i] + a * D[i]              VIP_NUMERICS_CPP (two roundings)
 *   w    = ws[ky,kx] * wc
 *   s    = fmaf(f_n, w, s)              VIP_NUMERICS_CUDA
 *   s    = s + f_n * w                  VIP_NUMERICS_CPP
 *   sumk = sumk + w
 *   dst  = s / sumk                     IEEE binary32 division, no clamp
 * Arithmetic is binary32 with gradual underflow (the kernels run in denormal mode 3, like their
 * siblings). sumk >= 1 always: the centre tap has t = 0 and wc = L[0] = 1.
 * Differences at or beyond value_range take the weight at value_range (t clamps to N): pass the
 * image's max - min for OpenCV's behaviour; a smaller value_range clamps, it does not fail.
 * Domain: every source value must be finite; the result then equals the definition bit for bit,
 * in both profiles (a difference that overflows to +Inf clamps like any other). With an Inf or NaN
 * in the source the values are unspecified, but the table index the kernel forms lies in [0, N]
 * for every bit pattern of the source (the tap's v_min_f32 returns N for a NaN), so such a call
 * reads nothing outside the table and cannot fault.
 * Tie to the 8-bit form: with value_range = 1024 (bin width exactly 1) and f == (float)g for a
 * gray u8 frame g, a is 0 at every tap, L[i] is the colour LUT's entry i bit for bit, and
 * u8(dst + 0.5f) is vip_bilateral_run_c1 on g.
 * ksize: odd, 1..vip_bilateral_f32_max_ksize() = 31 (VIP_ERR_UNSUPPORTED_KSIZE otherwise; the cap
 * has its own function, vip_max_ksize knows no id for this filter). ksize 1 returns f, except that
 * -0 becomes +0. Pitches are in bytes; d_src and d_dst bases and pitches must be multiples of 4,
 * and any such value works: 16-byte accesses where base and pitch are multiples of 16, dwords
 * otherwise. No byte of d_dst at column >= width or row >= out_rows is written.
 * VIP_ERR_INVALID_ARGUMENT: null handle or pointer, non-positive size, a bad band, a misaligned
 * base or pitch, a value_range that is not finite, not > 0, or gives a scale that is not finite
 * and > 0 (the sigmas are taken as vip_bilateral_create takes them); VIP_ERR_ALIASING: d_dst equals
 * d_src. One launch per call (vip::bilateral_f32_kernel<R, FMA>, R = ksize / 2), asynchronous, no
 * device allocation at run time; there is no runtime-radius kernel and vip_set_stencil_path does
 * not apply; the launch log and vip_kernel_timing_* see the kernel. The handle is read-only after
 * create. The _rows form takes a row band as vip_joint_bilateral_run_rows_f32. Measured times:
 * DESIGN.md section 4; nothing here promises a speed. */
#define VIP_BILATERAL_F32_BINS 1024
typedef struct vip_bilateral_f32_s* vip_bilateral_f32_t;
int vip_bilateral_f32_max_ksize(void);
int vip_bilateral_f32_create(vip_bilateral_f32_t* out, int width, int height, int ksize, float sigma_space,
                             float sigma_color, float value_range, int numerics);
int vip_bilateral_f32_destroy(vip_bilateral_f32_t h);
int vip_bilateral_f32_run(vip_bilateral_f32_t h, const float* d_src, size_t src_pitch, float* d_dst,
                          size_t dst_pitch, void* stream);
int vip_bilateral_f32_run_rows(vip_bilateral_f32_t h, const float* d_src, size_t src_pitch, float* d_dst,
                               size_t dst_pitch, int out_rows, int src_row0, int row_lo, int row_hi,
                               void* stream);
/* ---- self-guided bilateral filter of an f32 image of 2 or 3 interleaved channels: linear-light or
 * HDR RGB, a Lab frame, a normal map, a 2-channel flow field. The other half of OpenCV's CV_32F
 * bilateral (CV_32FC3): one range weight per tap, from the L1 distance over the channels, as the
 * 8-bit colour filter forms it. The handle is a vip_bilateral_f32_t as it stands: its tables scale,
 * L, D and ws are used exactly as above, and create knows nothing of the channel count.
 * The source is f_c(p), c = 0..C-1, C floats per pixel. Per output pixel the taps run in row-major
 * order over the k x k square, replicate border:
 *   d    = |f_0(n) - f_0(c)| + |f_1(n) - f_1(c)|                          C = 2
 *   d    = (|f_0(n) - f_0(c)| + |f_1(n) - f_1(c)|) + |f_2(n) - f_2(c)|    C = 3
 *           binary32 subtract, abs, then binary32 adds left to right
 *   t    = min(d * scale, (float)N);  i = (int)t;  a = t - (float)i
 *   wc   = fmaf(a, D[i], L[i])            VIP_NUMERICS_CUDA
 *   wc   = L[i] + a * D[i]                VIP_NUMERICS_CPP
 *   w    = ws[ky,kx] * wc                 formed once per tap
 *   s_c  = fmaf(f_c(n), w, s_c)  or  s_c + f_c(n) * w    for each channel
 *   sumk = sumk + w                       once per tap
 *   dst_c = s_c / sumk                    IEEE binary32 division
 * value_range is therefore the largest L1 distance that the N bins cover: a caller who wants
 * OpenCV's behaviour passes C * (max - min); a smaller value clamps (t = N), it does not fail.
 * Domain: as the one-channel filter's. Finite input gives the definition bit for bit in both
 * profiles; a sum of differences that overflows to +Inf clamps to N like any other. With a NaN or
 * Inf in the source the values are unspecified, but the table index lies in [0, N] for every bit
 * pattern: d * scale is the result of a multiply, and the tap's v_min_f32 returns N for a NaN.
 * Three identities follow. With value_range = 1024 and f == (float)g for a u8 3-channel frame g,
 * d <= 765, a is 0 at every tap and u8(dst_c + 0.5f) is vip_bilateral_run on g. If every channel
 * but channel 0 is constant over the frame, channel 0 of the result is vip_bilateral_f32_run on
 * plane 0 bit for bit (the other terms of d are exactly +0). ksize 1 returns f with -0 turned
 * into +0, per channel.
 * channels: 1, 2 or 3; anything else is VIP_ERR_INVALID_ARGUMENT. channels == 1 forwards to
 * vip_bilateral_f32_run / _run_rows (same kernels, same checks), so a caller generic over the
 * channel count needs no branch. Four channels are deliberately not offered: whether alpha takes
 * part in the distance has no agreed answer (filter the colour here and alpha on its own, or use
 * vip_joint_bilateral_run_f32c under a guide).
 * ksize: vip_bilateral_f32_max_ksize_c(channels) is 31 for 1 channel, 15 for 2 and 3, and 0 for any
 * other count; a handle whose ksize is above the cap for the given channel count gives
 * VIP_ERR_UNSUPPORTED_KSIZE at run. Every other rule is the one-channel filter's: pitches are in
 * bytes and at least width * channels * 4 (VIP_ERR_INVALID_ARGUMENT otherwise); d_src and d_dst
 * bases and pitches must be multiples of 4; 16-byte accesses are used only where base and pitch are
 * multiples of 16, decided separately for source and destination; no byte of d_dst is written at a
 * byte offset >= width * channels * 4 within a row, nor at a row >= out_rows; VIP_ERR_ALIASING when
 * d_dst equals d_src. One launch per call (vip::bilateral_f32c_kernel<R, C, FMA>, R = ksize / 2 in
 * 1..7; vip::bilateral_f32c_k1_kernel<C, FMA> for ksize 1), asynchronous, no device allocation; the
 * launch log and vip_kernel_timing_* see the kernel. The _rows form takes the band of
 * vip_bilateral_f32_run_rows. Measured times: DESIGN.md section 4; nothing here promises a speed. */
int vip_bilateral_f32_max_ksize_c(int channels);
int vip_bilateral_f32_run_c(vip_bilateral_f32_t h, const float* d_src, size_t src_pitch, int channels,
                            float* d_dst, size_t dst_pitch, void* stream);
int vip_bilateral_f32_run_rows_c(vip_bilateral_f32_t h, const float* d_src, size_t src_pitch, int channels,
                                 float* d_dst, size_t dst_pitch, int out_rows, int src_row0, int row_lo,
                                 int row_hi, void* stream);
/* ---- joint bilateral filter of an f32 one-channel source f under an f32 one-channel guide g of the
 * same size (no counterpart in the reference's API; OpenCV's ximgproc::jointBilateralFilter takes
 * CV_32F guides): a noisy depth or disparity map under an HDR or linear-light luminance plane, a
 * flow component or a matte under a depth map, a path-traced radiance plane under its depth
 * buffer. The handle is a vip_bilateral_f32_t as vip_bilateral_f32_create makes it: the same
 * scale, L, D and ws, N = VIP_BILATERAL_F32_BINS. value_range is the span of guide differences
 * the bins cover. Per output pixel the taps run in row-major order over the k x k square, with a
 * replicate border on both images:
 *   d    = |g_n - g_c|                  binary32 subtract, then abs
 *   t    = min(d * scale, (float)N)
 *   i    = (int)t;  a = t - (float)i    (exact)
 *   wc   = fmaf(a, D[i], L[i])          VIP_NUMERICS_CUDA
 *   wc   = L[i] + a * D[i]              VIP_NUMERICS_CPP (two roundings)
 *   w    = ws[ky,kx] * wc
 *   s    = fmaf(f_n, w, s)              VIP_NUMERICS_CUDA
 *   s    = s + f_n * w                  VIP_NUMERICS_CPP
 *   sumk = sumk + w
 *   dst  = s / sumk                     IEEE binary32 division, no clamp
 * Arithmetic is binary32 with gradual underflow; sumk >= 1 always (the centre tap has wc = L[0] = 1).
 * Domain: f and g must be finite; the result then equals the definition bit for bit, in both
 * profiles. With an Inf or NaN anywhere the values are unspecified, but the table index the kernel
 * forms lies in [0, N] for every bit pattern of the guide (d * scale is a product, and the tap's
 * v_min_f32 returns N for a NaN), and no address is formed from the source, so such a call reads
 * nothing outside the table and cannot fault.
 * Ties: with g == f the result is vip_bilateral_f32_run's bit for bit. With value_range = 1024 (bin
 * width exactly 1) and g == (float)g8 for a gray u8 frame g8, a is 0 at every tap, L[i] is the
 * colour LUT's entry i, and the result is vip_joint_bilateral_run_f32 under g8 (guide_channels 1)
 * bit for bit at the same sigmas.
 * ksize: odd, 1..vip_bilateral_f32_max_ksize_joint() = 31; a handle whose ksize is above the cap
 * gives VIP_ERR_UNSUPPORTED_KSIZE at run. ksize 1 returns f, except that -0 becomes +0, and does
 * not read the guide. Pitches are in bytes and at least width * 4; bases and pitches of d_src,
 * d_guide and d_dst must be multiples of 4, and any such value works: 16-byte accesses are used
 * only where a buffer's base and pitch are multiples of 16, decided for source, guide and
 * destination each on its own. No byte of d_dst at column >= width or row >= out_rows is written.
 * The _rows form takes a row band as vip_bilateral_f32_run_rows; rows of both images clamp into
 * [row_lo, row_hi). VIP_ERR_INVALID_ARGUMENT: null handle or pointer (a null guide too), a bad
 * band, a misaligned base or pitch, a pitch below width * 4; VIP_ERR_ALIASING: d_dst equals d_src
 * or d_guide. d_guide == d_src is allowed: it gives the self-guided result and still launches this
 * filter's kernel. One launch per call (vip::bilateral_f32_joint_kernel<R, FMA>, R = ksize / 2),
 * asynchronous, no device allocation; the launch log and vip_kernel_timing_* see the kernel.
 * Measured times: DESIGN.md section 4; nothing here promises a speed. */
int vip_bilateral_f32_max_ksize_joint(void);
int vip_bilateral_f32_run_joint(vip_bilateral_f32_t h, const float* d_src, size_t src_pitch,
                                const float* d_guide, size_t guide_pitch, float* d_dst, size_t dst_pitch,
                                void* stream);
int vip_bilateral_f32_run_rows_joint(vip_bilateral_f32_t h, const float* d_src, size_t src_pitch,
                                     const float* d_guide, size_t guide_pitch, float* d_dst, size_t dst_pitch,
                                     int out_rows, int src_row0, int row_lo, int row_hi, void* stream);
/* ---- joint bilateral upsampling (Kopf et al. 2007; no counterpart in the reference's API): a
 * field f solved at 1/2, 1/4 or 1/8 scale is brought up to the frame under the full-resolution
 * image, in one launch, with no full-resolution float intermediate.
 * Inputs and sizes: W x H is the output size, the full-resolution guide's. The scale s is 2, 4 or
 * 8. The low-resolution size is w = ceil(W / s), h = ceil(H / s) (vip_upsample_low_size). f is
 * w x h float32 with finite values. g is the w x h low-resolution guide, u8 with 1 or 3
 * interleaved channels; the caller supplies it: it is the image the field was solved on, whether
 * a subsample or an area average; the library does not derive it. G is the W x H full-resolution
 * guide with the same channel count. R = ksize / 2, ksize odd, 1..9, in low-resolution pixels.
 * Per output pixel (x, y): cx = x / s, px = x % s, cy = y / s, py = y % s, in integer
 * arithmetic. The taps run in row-major order over ky, kx in [-R, R]: the whole square, no disc.
 *   ix   = clamp(cx + kx, 0, w - 1),  iy = clamp(cy + ky, 0, h - 1)
 *   ox   = 2 s kx + (s - 1) - 2 px,   oy likewise
 *          (the offset from the output pixel to the centre of low-resolution cell cx + kx, in
 *          half full-resolution pixels: integers, symmetric in the phase)
 *   wsp  = space_weight(ox^2 + oy^2, 2 s sigma_space)
 *          (the function every handle's spatial LUT is built with: exp(-r2 / (2 sigma^2)), float
 *          or double coefficient by profile; 2 s sigma_space is an exact float product, so
 *          sigma_space is in low-resolution pixels)
 *   d    = |g(ix,iy) - G(x,y)|      (guide_channels 1)
 *        = |dB| + |dG| + |dR|       (guide_channels 3; the 768-entry colour LUT wc of sigma_color)
 *   wgt  = wsp * wc[d]              (one binary32 product)
 *   s    = fmaf(f(ix,iy), wgt, s)   VIP_NUMERICS_CUDA
 *   s    = s + f(ix,iy) * wgt       VIP_NUMERICS_CPP
 *   sumk = sumk + wgt
 *   dst(x,y) = sumk == 0 ? f(cx, cy) : s / sumk
 * Arithmetic is binary32 with gradual underflow (the kernels run in denormal mode 3 like their
 * siblings). No tap has weight 1, so sumk may be subnormal: the division is IEEE. sumk may also
 * be exactly zero, when every wc[d] has underflowed: then the nearest low-resolution sample is
 * returned (cx <= w - 1 always, so no clamp is needed). An Inf or NaN in f gives unspecified
 * values but can never fault: every address comes from coordinates and guides.
 * The handle holds the colour LUT and the device table of spatial weights and is read-only
 * after create: it may run on several streams at once. Each call is one launch
 * (vip::upsample_f32_kernel<R, S, GUIDE, FMA>), asynchronous, with no device allocation; the
 * launch log and vip_kernel_timing_* see it. Pitches are in bytes. d_src_lo and d_dst need base
 * and pitch that are multiples of 4; 16-byte accesses are used only where base and pitch allow.
 * The guides may have any base and pitch. No byte of d_dst is written at column >= width or
 * row >= height. VIP_ERR_INVALID_ARGUMENT: a null handle or pointer, a non-positive size, a scale
 * not in {2, 4, 8}, guide_channels not 1 or 3, a misaligned float pointer or pitch, a pitch
 * smaller than a row; VIP_ERR_UNSUPPORTED_KSIZE: an even ksize or one above 9
 * (vip_max_ksize(VIP_FILTER_UPSAMPLE)); VIP_ERR_ALIASING: d_dst equals any input.
 * vip_set_stencil_path and the vip_bilateral_set_* knobs do not apply. */
int vip_upsample_create(vip_upsample_t* out, int width, int height, int scale, int ksize, float sigma_space,
                        float sigma_color, int numerics);
int vip_upsample_destroy(vip_upsample_t h);
int vip_upsample_low_size(int width, int height, int scale, int* low_width, int* low_height);
int vip_upsample_run_f32(vip_upsample_t h, const float* d_src_lo, size_t src_pitch, const uint8_t* d_guide_lo,
                         size_t guide_lo_pitch, const uint8_t* d_guide, size_t guide_pitch, int guide_channels,
                         float* d_dst, size_t dst_pitch, void* stream);
/* ---- vip_upsample_run_f32 on an interleaved low-resolution field of 2..4 channels (flow at 1/4
 * scale, normals, float colour, RGBA), in one launch on the same handle: the weights depend on the
 * guides alone, so they are formed once per tap and serve every channel.
 * d_src_lo is low_width x low_height x channels and d_dst width x height x channels, interleaved:
 * channel c of cell or pixel (x, y) is
 *   ((float*)(base + y * pitch))[x * channels + c]
 * The handle, the guides, the scale, wsp, wc, d, the clamped cells and the row-major tap order are
 * those of vip_upsample_run_f32. Per output pixel and tap:
 *   wgt  = wsp * wc[d]                   formed once
 *   s_c  = fmaf(f_c(ix,iy), wgt, s_c)    for each channel c, VIP_NUMERICS_CUDA
 *   s_c  = s_c + f_c(ix,iy) * wgt        for each channel c, VIP_NUMERICS_CPP (two roundings)
 *   sumk = sumk + wgt                    once
 *   dst_c(x,y) = sumk == 0 ? f_c(cx, cy) : s_c / sumk
 * Arithmetic is binary32 with gradual underflow (denormal mode 3, as the sibling kernels).
 * Tie that holds bit for bit: for every c, plane c of dst is what vip_upsample_run_f32 writes for
 * plane c of the source, in both profiles, with both guide forms and at every scale, signed
 * zeros, subnormals and the sumk == 0 fallback included. With an Inf or NaN in the source the
 * values are unspecified, but the call cannot fault: no source value forms an address.
 * channels 1 forwards to vip_upsample_run_f32 (the same kernels, the same checks), so a caller
 * generic over the channel count needs no branch. channels 2, 3 and 4 take every scale and every
 * ksize the handle can have (odd, 1..9): there is no channel-dependent cap.
 * Pitches are in bytes. The float bases and pitches must be multiples of 4; 16-byte accesses are
 * used only where base and pitch are multiples of 16, decided separately for d_src_lo and d_dst.
 * The guides may have any base and pitch. No byte of d_dst is written at a byte offset
 * >= width * channels * 4 within a row, nor at a row >= height.
 * VIP_ERR_INVALID_ARGUMENT: a null handle or pointer; channels outside 1..4; guide_channels not 1
 * or 3; a misaligned float base or pitch; a pitch smaller than a row. VIP_ERR_ALIASING: d_dst
 * equals any input. One launch per call (vip::upsample_f32c_kernel<R, S, C, GUIDE, FMA>),
 * asynchronous, no device allocation; the launch log and vip_kernel_timing_* see it. Against C
 * launches of vip_upsample_run_f32 on de-interleaved planes: see DESIGN.md section 4; nothing
 * here promises a speed. */
int vip_upsample_run_f32c(vip_upsample_t h, const float* d_src_lo, size_t src_pitch, int channels,
                          const uint8_t* d_guide_lo, size_t guide_lo_pitch, const uint8_t* d_guide,
                          size_t guide_pitch, int guide_channels, float* d_dst, size_t dst_pitch, void* stream);
/* Tuning knob, process-wide (no reference counterpart): waves per workgroup of the plain
 * bilateral kernel for radius <= 8. 0 (default) = chosen per launch from the frame's
 * tile count (small frames take 8 or 4 waves and smaller tiles so more CUs work);
 * 16, 8 or 4 forces one. Results are identical for every setting (only the tiling
 * changes). The environment variable VIP_BIL_WAVES sets the initial value. */
int vip_bilateral_set_waves(int waves);
/* Companion knob: the tile shape of the same kernel for radius <= 8. 0 (default) = chosen
 * per launch with the wave count (small frames and the slabs of a frame split over many
 * GPUs take 256-pixel tiles, one row per wave and 4 outputs per thread: half the serial
 * work per thread); 1 forces 128-pixel tiles (4 rows per wave, 8 outputs per thread),
 * 2 forces 256-pixel tiles. Results are identical for every setting. The environment
 * variable VIP_BIL_WIDE sets the initial value. A forced wave count with mode 0 keeps
 * 128-pixel tiles. */
int vip_bilateral_set_wide(int mode);
/* Frames in flight the same choice plans for: 0 (default) = counted per device from the
 * distinct streams among its last 8 plain-bilateral launches (at most 4), so frames in
 * flight on several streams each get a tiling sized for their share of the CUs; 1..4 forces
 * the count (a measurement knob: e.g. timing one frame alone with the tiling the in-flight
 * frames use). The count is of streams, not of launches outstanding: a caller that
 * alternates streams but waits for each frame counts 2 or more too, and should force 1.
 * Results are identical for every setting. */
int vip_bilateral_set_frames_in_flight(int n);

/* ---- adaptive bilateral: CudaAdaptiveBilateralFilter
 *      (include/cuda/adaptive_bilateral_filter.hpp:9-19, src/adaptive_bilateral_filter_impl.cu:117-191) ---- */
int vip_adaptive_create(vip_adaptive_t* out, int width, int height, int ksize, float sigma_space, float sigma_color,
                        int numerics);
int vip_adaptive_destroy(vip_adaptive_t h);
int vip_adaptive_run(vip_adaptive_t h, const uint8_t* d_src, size_t src_pitch, uint8_t* d_dst, size_t dst_pitch,
                     void* stream);
int vip_adaptive_run_rows(vip_adaptive_t h, const uint8_t* d_src, size_t src_pitch, uint8_t* d_dst, size_t dst_pitch,
                          int out_rows, int src_row0, int row_lo, int row_hi, void* stream);
/* n frames per launch (up to 6), as vip_bilateral_run_rows_batch */
int vip_adaptive_run_rows_batch(vip_adaptive_t h, int n, const uint8_t* const* d_srcs, size_t src_pitch,
                                uint8_t* const* d_dsts, size_t dst_pitch, int out_rows, int src_row0, int row_lo,
                                int row_hi, int free_cus, void* stream);
/* ---- single-channel (8-bit gray) form (no reference counterpart). d_src and d_dst are one
 * byte per pixel; the handle is the same vip_adaptive_t, with its spatial LUT and its colour
 * LUT, of which one channel reaches only the first 511 entries. Per output pixel, replicate
 * border, radius = ksize / 2:
 *   mean = (float)(sum of g over the full k x k square) / (float)(k * k);  o = (float)c - mean
 *   per tap in row-major order over the k x k square:
 *     dist = |((float)n - (float)c) - o|;  w = ws[ky,kx] * wc[(int)dist]
 *     s += n * w (fused in the CUDA profile);  sumk += w
 *   dst = u8(s / sumk + 0.5f)
 * dist = |n - 2c + mean| <= 510 for every input. The result is, bit for bit, channel 0 of
 * vip_adaptive_run on the frame (g, 0, 0): channels 1 and 2 add exact zeros to dist. ksize
 * 1..63 odd. Any base address and pitch work for d_src and d_dst: the kernels use dword
 * loads / word stores only where the addresses allow, and never write a byte of d_dst at
 * column >= width or row >= out_rows (row padding stays the caller's). One launch per call,
 * no device allocation, no intermediate 3-channel buffer. VIP_ERR_INVALID_ARGUMENT: null
 * handle or pointer, a bad band; VIP_ERR_ALIASING: d_dst equals d_src. vip_set_stencil_path is
 * honoured (AUTO: radius-specialised vip::gray_adaptive_kernel for radius 1..15,
 * vip::gray_adaptive_rt_kernel for 0 and 16..31; RUNTIME: gray_adaptive_rt_kernel always).
 * There is no multi-frame (batch) form, and the vip_bilateral_set_* knobs do not apply. */
int vip_adaptive_run_c1(vip_adaptive_t h, const uint8_t* d_src, size_t src_pitch, uint8_t* d_dst, size_t dst_pitch,
                        void* stream);
/* Row band, as vip_adaptive_run_rows */
int vip_adaptive_run_rows_c1(vip_adaptive_t h, const uint8_t* d_src, size_t src_pitch, uint8_t* d_dst,
                             size_t dst_pitch, int out_rows, int src_row0, int row_lo, int row_hi, void* stream);

/* ---- gradient magnitude: cuda_gradient<T> (include/cuda/gradient.hpp:4-23, src/gradient_impl.cu:90-112) ---- */
int vip_gradient_u8(const uint8_t* d_src, float* d_dst, int width, int height, int src_ch, int numerics,
                    void* stream);
int vip_gradient_f32(const float* d_src, float* d_dst, int width, int height, int src_ch, int numerics,
                     void* stream);

/* ---- bilateral texture filter: CudaBilateralTextureFilter
 *      (include/cuda/bilateral_texture_filter.hpp:7-17, src/bilateral_texture_filter_impl.cu:179-275) ---- */
int vip_texture_create(vip_texture_t* out, int width, int height, int ksize, int nitr, int numerics);
int vip_texture_destroy(vip_texture_t h);
/* Device bytes a texture handle of this frame size allocates for its frames: two
 * ping-pong frames and the guide, u8x3 each (the reference's Impl also held f32
 * magnitude, blurred and rtv buffers, 20 B/px; no f32 scratch is held here). */
size_t vip_texture_scratch_bytes(int width, int height);
/* Impl::execute (:199-214); d_src and d_dst are dense width*3. The handle owns scratch
 * frames (like the reference's Impl): runs on one handle must not overlap, so frames in
 * flight on several streams take one handle per stream. Bilateral and adaptive handles
 * hold only read-only LUTs and may run on several streams at once. */
int vip_texture_run(vip_texture_t h, const uint8_t* d_src, uint8_t* d_dst, void* stream);
/* vip_texture_run with per-stage timestamps (measurement; no reference counterpart):
 * `events` holds 2*nitr + 1 hipEvent_t (created with timing enabled, passed as void*);
 * events[2i] is recorded on `stream` before iteration i's guide stage, events[2i+1]
 * before its joint bilateral, events[2*nitr] after the last launch. */
int vip_texture_run_timed(vip_texture_t h, const uint8_t* d_src, uint8_t* d_dst, void* stream, void* const* events);

/* Iteration form (no reference counterpart; same bytes either way). TWO_LAUNCH (the
 * default): per iteration the fused guide stage writes the guide frame to HBM and the
 * joint bilateral reads it -- src/bilateral_texture_filter_impl.cu:207-210's four stages
 * in two launches. FUSED (ksize 5 only, else VIP_ERR_UNSUPPORTED_KSIZE): one launch per
 * iteration, the guide of each JBF tile computed in LDS with the JBF apron (SURVEY
 * §8(f)1); vip_texture_run_timed's events[2i+1] then follows the whole iteration. The
 * row-slab entry point below always uses TWO_LAUNCH. */
#define VIP_TEXTURE_TWO_LAUNCH 0
#define VIP_TEXTURE_FUSED 1
int vip_texture_set_mode(vip_texture_t h, int mode);

/* ---- single-channel (8-bit gray) form (no reference counterpart). d_src and d_dst are one
 * byte per pixel; the handle is the same vip_texture_t (ksize 1..24, even too). The result is,
 * bit for bit, any channel of vip_texture_run on the frame (g, g, g): on a frame with three
 * equal channels every stage produces three equal channels. It is NOT the (g, 0, 0) embedding
 * of the gray bilateral and adaptive forms: the texture filter couples the channels in the
 * intensity (b + g + r) / 3.f, in the gradient magnitude and in the guide's L1 distance, so
 * (g, 0, 0) is a different image (its rtv is a third). One iteration on X, replicate border,
 * R = ksize / 2, window K = 2R + 1 (divisions by ksize^2 even for even ksize):
 *   mag       = sqrtf((float)(3 * (h*h + v*v))),  h = X(x+1,y) - X(x-1,y), v likewise (the exact
 *               integer sum over three equal channels, not sqrt(3) times a one-channel magnitude)
 *   intensity = (3 g) / 3.f == (float)g, so imax / imin are the integer max / min of g over the
 *               window (initial values 0 and 256)
 *   blurred   = (float)(sum of g over the window) / (ksize * ksize)
 *   rtv       = (imax - imin) * max(mag) / (sum(mag) + 1e-9), the sum in row-major order; the
 *               divide in double in the CUDA profile, in float with 1e-9f in the CPP profile
 *   G         = u8(alpha * blurred(min) + (1 - alpha) * blurred(c) + 0.5f) clamped to 0..255
 *               (fused in the CUDA profile), min the first strict argmin of rtv over the window,
 *               alpha = 2 / (1 + exp(sigma_alpha * (rtv(c) - rtv(min)))) - 1, sigma_alpha = 1 / (5 ksize)
 *   X'        = the joint bilateral of X under the gray guide G, ksize 2k - 1, sigma_space k - 1:
 *               w = ws[ky,kx] * wc[3 * |G_n - G_c|] with wc the 768-entry LUT of sigma_color
 *               sqrt(3) (3 * 255 = 765 lies inside it), sums as vip_joint_bilateral_run_c1
 * Iteration i reads X_i and writes X_{i+1}; the intermediates and the guide live in the
 * handle's scratch frames (no allocation per call; vip_texture_scratch_bytes is unchanged).
 * Two launches per iteration (vip::gray_texture_guide_kernel, then vip::gray_kernel with a gray
 * guide for k <= 16 or vip::gray_rt_kernel above and under VIP_PATH_RUNTIME);
 * vip_texture_set_mode is ignored. nitr 0 copies width bytes per row. d_dst == d_src with
 * equal pitches is allowed (through a scratch copy). Any base address and pitch work for d_src
 * and d_dst; no byte of d_dst at column >= width is written. VIP_ERR_INVALID_ARGUMENT: null
 * handle or pointer, a pitch < width. There is no row-slab, sharded or one-launch form, and no
 * one-channel vip_texture_blur_rtv / vip_texture_guide. */
int vip_texture_run_c1(vip_texture_t h, const uint8_t* d_src, size_t src_pitch, uint8_t* d_dst, size_t dst_pitch,
                       void* stream);

/* Row-slab form of one texture iteration for a row-sharded frame (SURVEY §8(f)3;
 * the reference is single-GPU). d_src is a dense slab of the handle's width x
 * height (pitch width*3) whose rows [row_lo, row_hi) are valid frame rows: every
 * stage clamps into them, which at a frame edge is the reference's replicate
 * border. Writes the iteration's rows [out_row0, out_row0 + out_rows) to d_dst
 * (row 0 of d_dst = slab row out_row0). Rows further than vip_texture_halo_rows(k)
 * from the frame edge must be backed by valid neighbour rows in d_src. */
int vip_texture_halo_rows(int ksize);
int vip_texture_iterate_rows(vip_texture_t h, const uint8_t* d_src, uint8_t* d_dst, size_t dst_pitch, int out_row0,
                             int out_rows, int row_lo, int row_hi, void* stream);
/* Impl::compute_blur_and_rtv (:216-237): image u8x3, magnitude f32 -> blurred f32x3, rtv f32 */
int vip_texture_blur_rtv(vip_texture_t h, const uint8_t* d_image, const float* d_magnitude, float* d_blurred,
                         float* d_rtv, void* stream);
/* Impl::compute_guide (:239-256): blurred f32x3, rtv f32 -> guide u8x3 */
int vip_texture_guide(vip_texture_t h, const float* d_blurred, const float* d_rtv, uint8_t* d_guide, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* VIP_H */
