// Drop-in for the reference's include/cuda/bilateral_filter.hpp:7-29.
// Same class name, constructor defaults and member signatures, so
// sample/bilateral_filter/main.cpp and test/bilateral_filter.cu compile against it.
// Backed by the C ABI in include/vip.h (libvip_hip.so, gfx950 HIP kernels).
// Pointers are device pointers to dense width*3 uint8 images; public calls block
// until the GPU is done (the reference synchronised the device, :299, :309).
#ifndef VIP_CUDA_BILATERAL_FILTER_HPP
#define VIP_CUDA_BILATERAL_FILTER_HPP

#include <cstdint>
#include <memory>

class CudaBilateralFilter {
public:
    CudaBilateralFilter(const int width, const int height, const int ksize = 9, const float sigma_space = 10.f,
                        const float sigma_color = 30.f);
    ~CudaBilateralFilter();

    void bilateral_filter(const std::uint8_t* const d_src, std::uint8_t* const d_dst) const;

    void joint_bilateral_filter(const std::uint8_t* const d_src, const std::uint8_t* const d_guide,
                                std::uint8_t* const d_dst) const;

    // Additive, non-blocking overloads: enqueue on `stream` (a
    // hipStream_t passed as void*, nullptr = default stream) and return at once.
    void bilateral_filter(const std::uint8_t* const d_src, std::uint8_t* const d_dst, void* stream) const;
    void joint_bilateral_filter(const std::uint8_t* const d_src, const std::uint8_t* const d_guide,
                                std::uint8_t* const d_dst, void* stream) const;

    // Additive one-channel (8-bit gray) forms, no reference counterpart (include/vip.h
    // vip_bilateral_run_c1): d_src and d_dst are dense width x height bytes; d_guide is dense gray
    // (guide_channels 1) or interleaved 3-channel (guide_channels 3). Blocking, and with a
    // stream non-blocking, as the 3-channel forms above.
    void bilateral_filter_c1(const std::uint8_t* const d_src, std::uint8_t* const d_dst) const;
    void joint_bilateral_filter_c1(const std::uint8_t* const d_src, const std::uint8_t* const d_guide,
                                   const int guide_channels, std::uint8_t* const d_dst) const;
    void bilateral_filter_c1(const std::uint8_t* const d_src, std::uint8_t* const d_dst, void* stream) const;
    void joint_bilateral_filter_c1(const std::uint8_t* const d_src, const std::uint8_t* const d_guide,
                                   const int guide_channels, std::uint8_t* const d_dst, void* stream) const;

    // Additive f32 form, no reference counterpart (include/vip.h vip_joint_bilateral_run_f32): a
    // dense width x height float source and destination under a dense gray (guide_channels 1) or
    // interleaved 3-channel (guide_channels 3) 8-bit guide. Blocking, and with a stream non-blocking.
    void joint_bilateral_filter_f32(const float* const d_src, const std::uint8_t* const d_guide,
                                    const int guide_channels, float* const d_dst) const;
    void joint_bilateral_filter_f32(const float* const d_src, const std::uint8_t* const d_guide,
                                    const int guide_channels, float* const d_dst, void* stream) const;

    // Confidence-weighted f32 form, which fills holes (include/vip.h
    // vip_joint_bilateral_run_conf_f32): d_conf is a dense width x height float confidence
    // (>= 0; 0 marks a hole, whose d_src value is ignored), hole_value what d_dst gets where no
    // weight was in reach, d_weight (optional) the dense float sum of weights. ksize <= 31.
    // Blocking, and with a stream non-blocking.
    void joint_bilateral_filter_conf_f32(const float* const d_src, const float* const d_conf,
                                         const std::uint8_t* const d_guide, const int guide_channels,
                                         const float hole_value, float* const d_dst,
                                         float* const d_weight = nullptr) const;
    void joint_bilateral_filter_conf_f32(const float* const d_src, const float* const d_conf,
                                         const std::uint8_t* const d_guide, const int guide_channels,
                                         const float hole_value, float* const d_dst, float* const d_weight,
                                         void* stream) const;

    // The f32 form on an interleaved source of 1..4 channels (include/vip.h
    // vip_joint_bilateral_run_f32c): d_src and d_dst are dense width x height x channels floats,
    // every channel filtered under the same guide in one launch. ksize <= 47 / 31 / 15 / 15 for
    // 1 / 2 / 3 / 4 channels. Blocking, and with a stream non-blocking.
    void joint_bilateral_filter_f32c(const float* const d_src, const int channels, const std::uint8_t* const d_guide,
                                     const int guide_channels, float* const d_dst) const;
    void joint_bilateral_filter_f32c(const float* const d_src, const int channels, const std::uint8_t* const d_guide,
                                     const int guide_channels, float* const d_dst, void* stream) const;

protected:
    class Impl;  // defined in bilateral_filter_impl.cuh (test drivers reach it through impl_)
    std::unique_ptr<Impl> impl_;
};

#endif  // VIP_CUDA_BILATERAL_FILTER_HPP
