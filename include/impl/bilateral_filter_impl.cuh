// Impl of CudaBilateralFilter, visible to test drivers the way the reference's
// src/bilateral_filter_impl.cuh:7-33 is (test/bilateral_filter.cu:9-33 subclasses
// the public class and calls impl_->bilateral_filter without a device sync).
// Methods here are asynchronous on the default stream.
#ifndef VIP_IMPL_BILATERAL_FILTER_IMPL_CUH
#define VIP_IMPL_BILATERAL_FILTER_IMPL_CUH

#include <cstdint>

#include "cuda/bilateral_filter.hpp"
#include "vip.h"

class CudaBilateralFilter::Impl {
public:
    Impl(const int width, const int height, const int ksize = 9, const float sigma_space = 10.f,
         const float sigma_color = 30.f);
    ~Impl();
    Impl(const Impl&) = delete;
    Impl& operator=(const Impl&) = delete;

    void bilateral_filter(const std::uint8_t* const d_src, std::uint8_t* const d_dst) const;
    void joint_bilateral_filter(const std::uint8_t* const d_src, const std::uint8_t* const d_guide,
                                std::uint8_t* const d_dst) const;
    void bilateral_filter(const std::uint8_t* const d_src, std::uint8_t* const d_dst, void* stream) const;
    void joint_bilateral_filter(const std::uint8_t* const d_src, const std::uint8_t* const d_guide,
                                std::uint8_t* const d_dst, void* stream) const;

    // one-channel forms (include/cuda/bilateral_filter.hpp)
    void bilateral_filter_c1(const std::uint8_t* const d_src, std::uint8_t* const d_dst) const;
    void joint_bilateral_filter_c1(const std::uint8_t* const d_src, const std::uint8_t* const d_guide,
                                   const int guide_channels, std::uint8_t* const d_dst) const;
    void bilateral_filter_c1(const std::uint8_t* const d_src, std::uint8_t* const d_dst, void* stream) const;
    void joint_bilateral_filter_c1(const std::uint8_t* const d_src, const std::uint8_t* const d_guide,
                                   const int guide_channels, std::uint8_t* const d_dst, void* stream) const;

    // f32 source under an 8-bit guide (include/cuda/bilateral_filter.hpp)
    void joint_bilateral_filter_f32(const float* const d_src, const std::uint8_t* const d_guide,
                                    const int guide_channels, float* const d_dst) const;
    void joint_bilateral_filter_f32(const float* const d_src, const std::uint8_t* const d_guide,
                                    const int guide_channels, float* const d_dst, void* stream) const;
    // confidence-weighted f32 form (stream-ordered; the class's blocking overload synchronises)
    void joint_bilateral_filter_conf_f32(const float* const d_src, const float* const d_conf,
                                         const std::uint8_t* const d_guide, const int guide_channels,
                                         const float hole_value, float* const d_dst, float* const d_weight,
                                         void* stream) const;
    // the f32 form on 1..4 interleaved channels (stream-ordered; the class's blocking overload synchronises)
    void joint_bilateral_filter_f32c(const float* const d_src, const int channels, const std::uint8_t* const d_guide,
                                     const int guide_channels, float* const d_dst, void* stream) const;

    vip_bilateral_t handle() const { return handle_; }

private:
    const int width_;
    vip_bilateral_t handle_ = nullptr;
};

#endif  // VIP_IMPL_BILATERAL_FILTER_IMPL_CUH
