// Joint bilateral upsampling of a low-resolution f32 field under an 8-bit guide (Kopf et al.
// 2007); no reference counterpart. Backed by the C ABI in include/vip.h (vip_upsample_*,
// libvip_hip.so, gfx950 HIP kernels), which holds the definition.
// Pointers are device pointers to dense images: d_src_lo low_width() x low_height() floats,
// d_guide_lo the same size in bytes times guide_channels (1: gray, 3: interleaved), d_guide
// width x height x guide_channels bytes, d_dst width x height floats; upsample_f32c takes
// channels (1..4) interleaved floats per cell of d_src_lo and per pixel of d_dst
// (vip_upsample_run_f32c: each channel is upsample_f32 on its plane). The call without a stream
// blocks until the GPU is done, like the other classes' public calls; with a stream (a
// hipStream_t passed as void*, nullptr = default stream) it enqueues and returns at once.
#ifndef VIP_CUDA_JOINT_BILATERAL_UPSAMPLE_HPP
#define VIP_CUDA_JOINT_BILATERAL_UPSAMPLE_HPP

#include <cstdint>

struct vip_upsample_s;

class CudaJointBilateralUpsample {
public:
    // scale 2, 4 or 8; ksize odd, 1..9, and sigma_space in low-resolution pixels
    CudaJointBilateralUpsample(const int width, const int height, const int scale, const int ksize = 5,
                               const float sigma_space = 1.f, const float sigma_color = 30.f);
    ~CudaJointBilateralUpsample();
    CudaJointBilateralUpsample(const CudaJointBilateralUpsample&) = delete;
    CudaJointBilateralUpsample& operator=(const CudaJointBilateralUpsample&) = delete;

    void upsample_f32(const float* const d_src_lo, const std::uint8_t* const d_guide_lo,
                      const std::uint8_t* const d_guide, const int guide_channels, float* const d_dst) const;
    void upsample_f32(const float* const d_src_lo, const std::uint8_t* const d_guide_lo,
                      const std::uint8_t* const d_guide, const int guide_channels, float* const d_dst,
                      void* stream) const;
    void upsample_f32c(const float* const d_src_lo, const int channels, const std::uint8_t* const d_guide_lo,
                       const std::uint8_t* const d_guide, const int guide_channels, float* const d_dst) const;
    void upsample_f32c(const float* const d_src_lo, const int channels, const std::uint8_t* const d_guide_lo,
                       const std::uint8_t* const d_guide, const int guide_channels, float* const d_dst,
                       void* stream) const;

    // ceil(width / scale), ceil(height / scale)
    int low_width() const { return low_width_; }
    int low_height() const { return low_height_; }

private:
    const int width_;
    int low_width_ = 0, low_height_ = 0;
    vip_upsample_s* handle_ = nullptr;
};

#endif  // VIP_CUDA_JOINT_BILATERAL_UPSAMPLE_HPP
