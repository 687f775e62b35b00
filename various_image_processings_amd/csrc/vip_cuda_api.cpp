// C++ drop-in API (include/cuda/*.hpp + include/impl/*.cuh) implemented over the
// C ABI. Error behaviour follows the reference's CUDASafeCall
// (src/host_utilities.hpp:9-13): print "HIP Error <file> : <line> <message>" to
// stderr and carry on; allocation failures in constructors throw
// std::runtime_error (thrust::device_vector threw std::bad_alloc in the reference).


#include <cstdio>
#include <stdexcept>
#include <string>

#include "cuda/bilateral_filter_f32.hpp"
#include "cuda/device_image.hpp"
#include "cuda/gradient.hpp"
#include "cuda/joint_bilateral_upsample.hpp"
#include "impl/adaptive_bilateral_filter_impl.cuh"
#include "impl/bilateral_filter_impl.cuh"
#include "impl/bilateral_texture_filter_impl.cuh"
#include "vip.h"

namespace {

void report(int rc, const char* file, int line) {
    if (rc != 0) std::fprintf(stderr, "HIP Error %s : %d %s\n", file, line, vip_error_string(rc));
}
#define VIP_REPORT(expr) report((expr), __FILE__, __LINE__)

[[noreturn]] void fail(const char* what, int rc) {
    throw std::runtime_error(std::string(what) + ": " + vip_error_string(rc));
}

}  // namespace

// ------------------------------------------------------------ CudaBilateralFilter
CudaBilateralFilter::Impl::Impl(const int width, const int height, const int ksize, const float sigma_space,
                                const float sigma_color)
    : width_(width) {
    (void)height;
    const int rc = vip_bilateral_create(&handle_, width, height, ksize, sigma_space, sigma_color, VIP_NUMERICS_CUDA);
    if (rc) fail("CudaBilateralFilter", rc);
}
CudaBilateralFilter::Impl::~Impl() { vip_bilateral_destroy(handle_); }

void CudaBilateralFilter::Impl::bilateral_filter(const std::uint8_t* const d_src, std::uint8_t* const d_dst) const {
    bilateral_filter(d_src, d_dst, nullptr);
}
void CudaBilateralFilter::Impl::bilateral_filter(const std::uint8_t* const d_src, std::uint8_t* const d_dst,
                                                 void* stream) const {
    VIP_REPORT(vip_bilateral_run(handle_, d_src, (size_t)width_ * 3, d_dst, (size_t)width_ * 3, stream));
}

void CudaBilateralFilter::Impl::joint_bilateral_filter(const std::uint8_t* const d_src,
                                                       const std::uint8_t* const d_guide,
                                                       std::uint8_t* const d_dst) const {
    joint_bilateral_filter(d_src, d_guide, d_dst, nullptr);
}
void CudaBilateralFilter::Impl::joint_bilateral_filter(const std::uint8_t* const d_src,
                                                       const std::uint8_t* const d_guide, std::uint8_t* const d_dst,
                                                       void* stream) const {
    const size_t pitch = (size_t)width_ * 3;
    VIP_REPORT(vip_joint_bilateral_run(handle_, d_src, pitch, d_guide, pitch, d_dst, pitch, stream));
}

void CudaBilateralFilter::Impl::bilateral_filter_c1(const std::uint8_t* const d_src, std::uint8_t* const d_dst) const {
    bilateral_filter_c1(d_src, d_dst, nullptr);
}
void CudaBilateralFilter::Impl::bilateral_filter_c1(const std::uint8_t* const d_src, std::uint8_t* const d_dst,
                                                    void* stream) const {
    VIP_REPORT(vip_bilateral_run_c1(handle_, d_src, (size_t)width_, d_dst, (size_t)width_, stream));
}
void CudaBilateralFilter::Impl::joint_bilateral_filter_c1(const std::uint8_t* const d_src,
                                                          const std::uint8_t* const d_guide, const int guide_channels,
                                                          std::uint8_t* const d_dst) const {
    joint_bilateral_filter_c1(d_src, d_guide, guide_channels, d_dst, nullptr);
}
void CudaBilateralFilter::Impl::joint_bilateral_filter_c1(const std::uint8_t* const d_src,
                                                          const std::uint8_t* const d_guide, const int guide_channels,
                                                          std::uint8_t* const d_dst, void* stream) const {
    const size_t pitch = (size_t)width_;
    VIP_REPORT(vip_joint_bilateral_run_c1(handle_, d_src, pitch, d_guide, pitch * (size_t)(guide_channels == 3 ? 3 : 1),
                                          guide_channels, d_dst, pitch, stream));
}

void CudaBilateralFilter::Impl::joint_bilateral_filter_f32(const float* const d_src, const std::uint8_t* const d_guide,
                                                           const int guide_channels, float* const d_dst) const {
    joint_bilateral_filter_f32(d_src, d_guide, guide_channels, d_dst, nullptr);
}
void CudaBilateralFilter::Impl::joint_bilateral_filter_f32(const float* const d_src, const std::uint8_t* const d_guide,
                                                           const int guide_channels, float* const d_dst,
                                                           void* stream) const {
    const size_t pitch = (size_t)width_;
    VIP_REPORT(vip_joint_bilateral_run_f32(handle_, d_src, pitch * sizeof(float), d_guide,
                                           pitch * (size_t)(guide_channels == 3 ? 3 : 1), guide_channels, d_dst,
                                           pitch * sizeof(float), stream));
}
void CudaBilateralFilter::Impl::joint_bilateral_filter_conf_f32(const float* const d_src, const float* const d_conf,
                                                                const std::uint8_t* const d_guide,
                                                                const int guide_channels, const float hole_value,
                                                                float* const d_dst, float* const d_weight,
                                                                void* stream) const {
    const size_t pitch = (size_t)width_, fp = pitch * sizeof(float);
    VIP_REPORT(vip_joint_bilateral_run_conf_f32(handle_, d_src, fp, d_conf, fp, d_guide,
                                                pitch * (size_t)(guide_channels == 3 ? 3 : 1), guide_channels,
                                                hole_value, d_dst, fp, d_weight, fp, stream));
}
void CudaBilateralFilter::Impl::joint_bilateral_filter_f32c(const float* const d_src, const int channels,
                                                            const std::uint8_t* const d_guide, const int guide_channels,
                                                            float* const d_dst, void* stream) const {
    const size_t pitch = (size_t)width_, fp = pitch * sizeof(float) * (size_t)(channels > 0 ? channels : 0);
    VIP_REPORT(vip_joint_bilateral_run_f32c(handle_, d_src, fp, channels, d_guide,
                                            pitch * (size_t)(guide_channels == 3 ? 3 : 1), guide_channels, d_dst, fp,
                                            stream));
}

CudaBilateralFilter::CudaBilateralFilter(const int width, const int height, const int ksize, const float sigma_space,
                                         const float sigma_color)
    : impl_(std::make_unique<Impl>(width, height, ksize, sigma_space, sigma_color)) {}
CudaBilateralFilter::~CudaBilateralFilter() = default;

void CudaBilateralFilter::bilateral_filter(const std::uint8_t* const d_src, std::uint8_t* const d_dst) const {
    impl_->bilateral_filter(d_src, d_dst);
    VIP_REPORT(vip_device_synchronize());
}

void CudaBilateralFilter::joint_bilateral_filter(const std::uint8_t* const d_src, const std::uint8_t* const d_guide,
                                                 std::uint8_t* const d_dst) const {
    impl_->joint_bilateral_filter(d_src, d_guide, d_dst);
    VIP_REPORT(vip_device_synchronize());
}

void CudaBilateralFilter::bilateral_filter(const std::uint8_t* const d_src, std::uint8_t* const d_dst,
                                           void* stream) const {
    impl_->bilateral_filter(d_src, d_dst, stream);
}

void CudaBilateralFilter::joint_bilateral_filter(const std::uint8_t* const d_src, const std::uint8_t* const d_guide,
                                                 std::uint8_t* const d_dst, void* stream) const {
    impl_->joint_bilateral_filter(d_src, d_guide, d_dst, stream);
}

void CudaBilateralFilter::bilateral_filter_c1(const std::uint8_t* const d_src, std::uint8_t* const d_dst) const {
    impl_->bilateral_filter_c1(d_src, d_dst);
    VIP_REPORT(vip_device_synchronize());
}
void CudaBilateralFilter::joint_bilateral_filter_c1(const std::uint8_t* const d_src, const std::uint8_t* const d_guide,
                                                    const int guide_channels, std::uint8_t* const d_dst) const {
    impl_->joint_bilateral_filter_c1(d_src, d_guide, guide_channels, d_dst);
    VIP_REPORT(vip_device_synchronize());
}
void CudaBilateralFilter::bilateral_filter_c1(const std::uint8_t* const d_src, std::uint8_t* const d_dst,
                                              void* stream) const {
    impl_->bilateral_filter_c1(d_src, d_dst, stream);
}
void CudaBilateralFilter::joint_bilateral_filter_c1(const std::uint8_t* const d_src, const std::uint8_t* const d_guide,
                                                    const int guide_channels, std::uint8_t* const d_dst,
                                                    void* stream) const {
    impl_->joint_bilateral_filter_c1(d_src, d_guide, guide_channels, d_dst, stream);
}
void CudaBilateralFilter::joint_bilateral_filter_f32(const float* const d_src, const std::uint8_t* const d_guide,
                                                     const int guide_channels, float* const d_dst) const {
    impl_->joint_bilateral_filter_f32(d_src, d_guide, guide_channels, d_dst);
    VIP_REPORT(vip_device_synchronize());
}
void CudaBilateralFilter::joint_bilateral_filter_f32(const float* const d_src, const std::uint8_t* const d_guide,
                                                     const int guide_channels, float* const d_dst,
                                                     void* stream) const {
    impl_->joint_bilateral_filter_f32(d_src, d_guide, guide_channels, d_dst, stream);
}
void CudaBilateralFilter::joint_bilateral_filter_conf_f32(const float* const d_src, const float* const d_conf,
                                                          const std::uint8_t* const d_guide, const int guide_channels,
                                                          const float hole_value, float* const d_dst,
                                                          float* const d_weight) const {
    impl_->joint_bilateral_filter_conf_f32(d_src, d_conf, d_guide, guide_channels, hole_value, d_dst, d_weight,
                                           nullptr);
    VIP_REPORT(vip_device_synchronize());
}
void CudaBilateralFilter::joint_bilateral_filter_conf_f32(const float* const d_src, const float* const d_conf,
                                                          const std::uint8_t* const d_guide, const int guide_channels,
                                                          const float hole_value, float* const d_dst,
                                                          float* const d_weight, void* stream) const {
    impl_->joint_bilateral_filter_conf_f32(d_src, d_conf, d_guide, guide_channels, hole_value, d_dst, d_weight,
                                           stream);
}
void CudaBilateralFilter::joint_bilateral_filter_f32c(const float* const d_src, const int channels,
                                                      const std::uint8_t* const d_guide, const int guide_channels,
                                                      float* const d_dst) const {
    impl_->joint_bilateral_filter_f32c(d_src, channels, d_guide, guide_channels, d_dst, nullptr);
    VIP_REPORT(vip_device_synchronize());
}
void CudaBilateralFilter::joint_bilateral_filter_f32c(const float* const d_src, const int channels,
                                                      const std::uint8_t* const d_guide, const int guide_channels,
                                                      float* const d_dst, void* stream) const {
    impl_->joint_bilateral_filter_f32c(d_src, channels, d_guide, guide_channels, d_dst, stream);
}

// ------------------------------------------------------------ CudaJointBilateralUpsample
CudaJointBilateralUpsample::CudaJointBilateralUpsample(const int width, const int height, const int scale,
                                                       const int ksize, const float sigma_space,
                                                       const float sigma_color)
    : width_(width) {
    int rc = vip_upsample_create(&handle_, width, height, scale, ksize, sigma_space, sigma_color, VIP_NUMERICS_CUDA);
    if (!rc) rc = vip_upsample_low_size(width, height, scale, &low_width_, &low_height_);
    if (rc) fail("CudaJointBilateralUpsample", rc);
}
CudaJointBilateralUpsample::~CudaJointBilateralUpsample() { vip_upsample_destroy(handle_); }

void CudaJointBilateralUpsample::upsample_f32(const float* const d_src_lo, const std::uint8_t* const d_guide_lo,
                                              const std::uint8_t* const d_guide, const int guide_channels,
                                              float* const d_dst, void* stream) const {
    const size_t gch = guide_channels == 3 ? 3 : 1;
    VIP_REPORT(vip_upsample_run_f32(handle_, d_src_lo, (size_t)low_width_ * sizeof(float), d_guide_lo,
                                    (size_t)low_width_ * gch, d_guide, (size_t)width_ * gch, guide_channels, d_dst,
                                    (size_t)width_ * sizeof(float), stream));
}
void CudaJointBilateralUpsample::upsample_f32(const float* const d_src_lo, const std::uint8_t* const d_guide_lo,
                                              const std::uint8_t* const d_guide, const int guide_channels,
                                              float* const d_dst) const {
    upsample_f32(d_src_lo, d_guide_lo, d_guide, guide_channels, d_dst, nullptr);
    VIP_REPORT(vip_device_synchronize());
}

void CudaJointBilateralUpsample::upsample_f32c(const float* const d_src_lo, const int channels,
                                               const std::uint8_t* const d_guide_lo,
                                               const std::uint8_t* const d_guide, const int guide_channels,
                                               float* const d_dst, void* stream) const {
    const size_t gch = guide_channels == 3 ? 3 : 1;
    const size_t cell = sizeof(float) * (size_t)(channels > 0 ? channels : 1);  // the C ABI refuses channels < 1
    VIP_REPORT(vip_upsample_run_f32c(handle_, d_src_lo, (size_t)low_width_ * cell, channels, d_guide_lo,
                                     (size_t)low_width_ * gch, d_guide, (size_t)width_ * gch, guide_channels, d_dst,
                                     (size_t)width_ * cell, stream));
}
void CudaJointBilateralUpsample::upsample_f32c(const float* const d_src_lo, const int channels,
                                               const std::uint8_t* const d_guide_lo,
                                               const std::uint8_t* const d_guide, const int guide_channels,
                                               float* const d_dst) const {
    upsample_f32c(d_src_lo, channels, d_guide_lo, d_guide, guide_channels, d_dst, nullptr);
    VIP_REPORT(vip_device_synchronize());
}

// ------------------------------------------------------------ CudaBilateralFilterF32
CudaBilateralFilterF32::Impl::Impl(const int width, const int height, const int ksize, const float sigma_space,
                                   const float sigma_color, const float value_range)
    : width_(width) {
    const int rc = vip_bilateral_f32_create(&handle_, width, height, ksize, sigma_space, sigma_color, value_range,
                                            VIP_NUMERICS_CUDA);
    if (rc) fail("CudaBilateralFilterF32", rc);
}
CudaBilateralFilterF32::Impl::~Impl() { vip_bilateral_f32_destroy(handle_); }

void CudaBilateralFilterF32::Impl::bilateral_filter(const float* const d_src, float* const d_dst, void* stream) const {
    const size_t pitch = (size_t)width_ * sizeof(float);
    VIP_REPORT(vip_bilateral_f32_run(handle_, d_src, pitch, d_dst, pitch, stream));
}
void CudaBilateralFilterF32::Impl::bilateral_filter(const float* const d_src, const int channels, float* const d_dst,
                                                    void* stream) const {
    const size_t pitch = (size_t)width_ * sizeof(float) * (size_t)(channels > 0 ? channels : 1);  // the C ABI refuses channels < 1
    VIP_REPORT(vip_bilateral_f32_run_c(handle_, d_src, pitch, channels, d_dst, pitch, stream));
}
void CudaBilateralFilterF32::Impl::joint_bilateral_filter(const float* const d_src, const float* const d_guide,
                                                          float* const d_dst, void* stream) const {
    const size_t pitch = (size_t)width_ * sizeof(float);
    VIP_REPORT(vip_bilateral_f32_run_joint(handle_, d_src, pitch, d_guide, pitch, d_dst, pitch, stream));
}

CudaBilateralFilterF32::CudaBilateralFilterF32(const int width, const int height, const int ksize,
                                               const float sigma_space, const float sigma_color,
                                               const float value_range)
    : impl_(std::make_unique<Impl>(width, height, ksize, sigma_space, sigma_color, value_range)) {}
CudaBilateralFilterF32::~CudaBilateralFilterF32() = default;

void CudaBilateralFilterF32::bilateral_filter(const float* const d_src, float* const d_dst, void* stream) const {
    impl_->bilateral_filter(d_src, d_dst, stream);
}
void CudaBilateralFilterF32::bilateral_filter(const float* const d_src, float* const d_dst) const {
    impl_->bilateral_filter(d_src, d_dst, nullptr);
    VIP_REPORT(vip_device_synchronize());
}
void CudaBilateralFilterF32::bilateral_filter(const float* const d_src, const int channels, float* const d_dst,
                                              void* stream) const {
    impl_->bilateral_filter(d_src, channels, d_dst, stream);
}
void CudaBilateralFilterF32::bilateral_filter(const float* const d_src, const int channels, float* const d_dst) const {
    impl_->bilateral_filter(d_src, channels, d_dst, nullptr);
    VIP_REPORT(vip_device_synchronize());
}
void CudaBilateralFilterF32::joint_bilateral_filter(const float* const d_src, const float* const d_guide,
                                                    float* const d_dst, void* stream) const {
    impl_->joint_bilateral_filter(d_src, d_guide, d_dst, stream);
}
void CudaBilateralFilterF32::joint_bilateral_filter(const float* const d_src, const float* const d_guide,
                                                    float* const d_dst) const {
    impl_->joint_bilateral_filter(d_src, d_guide, d_dst, nullptr);
    VIP_REPORT(vip_device_synchronize());
}

// ------------------------------------------------------------ CudaAdaptiveBilateralFilter
CudaAdaptiveBilateralFilter::Impl::Impl(const int width, const int height, const int ksize, const float sigma_space,
                                        const float sigma_color)
    : width_(width) {
    (void)height;
    const int rc = vip_adaptive_create(&handle_, width, height, ksize, sigma_space, sigma_color, VIP_NUMERICS_CUDA);
    if (rc) fail("CudaAdaptiveBilateralFilter", rc);
}
CudaAdaptiveBilateralFilter::Impl::~Impl() { vip_adaptive_destroy(handle_); }

void CudaAdaptiveBilateralFilter::Impl::execute(const std::uint8_t* const d_src, std::uint8_t* const d_dst) const {
    execute(d_src, d_dst, nullptr);
}
void CudaAdaptiveBilateralFilter::Impl::execute(const std::uint8_t* const d_src, std::uint8_t* const d_dst,
                                                void* stream) const {
    VIP_REPORT(vip_adaptive_run(handle_, d_src, (size_t)width_ * 3, d_dst, (size_t)width_ * 3, stream));
}
void CudaAdaptiveBilateralFilter::Impl::execute_c1(const std::uint8_t* const d_src, std::uint8_t* const d_dst) const {
    execute_c1(d_src, d_dst, nullptr);
}
void CudaAdaptiveBilateralFilter::Impl::execute_c1(const std::uint8_t* const d_src, std::uint8_t* const d_dst,
                                                   void* stream) const {
    VIP_REPORT(vip_adaptive_run_c1(handle_, d_src, (size_t)width_, d_dst, (size_t)width_, stream));
}

CudaAdaptiveBilateralFilter::CudaAdaptiveBilateralFilter(const int width, const int height, const int ksize,
                                                         const float sigma_space, const float sigma_color)
    : impl_(std::make_unique<Impl>(width, height, ksize, sigma_space, sigma_color)) {}
CudaAdaptiveBilateralFilter::~CudaAdaptiveBilateralFilter() = default;

void CudaAdaptiveBilateralFilter::execute(const std::uint8_t* const d_src, std::uint8_t* const d_dst) const {
    impl_->execute(d_src, d_dst);
    VIP_REPORT(vip_device_synchronize());
}

void CudaAdaptiveBilateralFilter::execute(const std::uint8_t* const d_src, std::uint8_t* const d_dst,
                                          void* stream) const {
    impl_->execute(d_src, d_dst, stream);
}

void CudaAdaptiveBilateralFilter::execute_c1(const std::uint8_t* const d_src, std::uint8_t* const d_dst) const {
    impl_->execute_c1(d_src, d_dst);
    VIP_REPORT(vip_device_synchronize());
}
void CudaAdaptiveBilateralFilter::execute_c1(const std::uint8_t* const d_src, std::uint8_t* const d_dst,
                                             void* stream) const {
    impl_->execute_c1(d_src, d_dst, stream);
}

// ------------------------------------------------------------ CudaBilateralTextureFilter
CudaBilateralTextureFilter::Impl::Impl(const int width, const int height, const int ksize, const int nitr)
    : width_(width) {
    const int rc = vip_texture_create(&handle_, width, height, ksize, nitr, VIP_NUMERICS_CUDA);
    if (rc) fail("CudaBilateralTextureFilter", rc);
}
CudaBilateralTextureFilter::Impl::~Impl() { vip_texture_destroy(handle_); }

void CudaBilateralTextureFilter::Impl::execute(const std::uint8_t* const d_src, std::uint8_t* const d_dst) {
    execute(d_src, d_dst, nullptr);
}
void CudaBilateralTextureFilter::Impl::execute(const std::uint8_t* const d_src, std::uint8_t* const d_dst,
                                               void* stream) {
    VIP_REPORT(vip_texture_run(handle_, d_src, d_dst, stream));
}
void CudaBilateralTextureFilter::Impl::execute_c1(const std::uint8_t* const d_src, std::uint8_t* const d_dst) {
    execute_c1(d_src, d_dst, nullptr);
}
void CudaBilateralTextureFilter::Impl::execute_c1(const std::uint8_t* const d_src, std::uint8_t* const d_dst,
                                                  void* stream) {
    VIP_REPORT(vip_texture_run_c1(handle_, d_src, (size_t)width_, d_dst, (size_t)width_, stream));
}

void CudaBilateralTextureFilter::Impl::compute_blur_and_rtv(const std::uint8_t* d_image, const float* d_magnitude,
                                                            float* d_blurred, float* d_rtv) {
    VIP_REPORT(vip_texture_blur_rtv(handle_, d_image, d_magnitude, d_blurred, d_rtv, nullptr));
}

void CudaBilateralTextureFilter::Impl::compute_guide(const float* d_blurred, const float* d_rtv,
                                                     std::uint8_t* d_guide) {
    VIP_REPORT(vip_texture_guide(handle_, d_blurred, d_rtv, d_guide, nullptr));
}

CudaBilateralTextureFilter::CudaBilateralTextureFilter(const int width, const int height, const int ksize,
                                                       const int nitr)
    : impl_(std::make_unique<Impl>(width, height, ksize, nitr)) {}
CudaBilateralTextureFilter::~CudaBilateralTextureFilter() = default;

void CudaBilateralTextureFilter::execute(const std::uint8_t* const d_src, std::uint8_t* const d_dst) {
    impl_->execute(d_src, d_dst);
    VIP_REPORT(vip_device_synchronize());
}

void CudaBilateralTextureFilter::execute(const std::uint8_t* const d_src, std::uint8_t* const d_dst, void* stream) {
    impl_->execute(d_src, d_dst, stream);
}

void CudaBilateralTextureFilter::execute_c1(const std::uint8_t* const d_src, std::uint8_t* const d_dst) {
    impl_->execute_c1(d_src, d_dst);
    VIP_REPORT(vip_device_synchronize());
}
void CudaBilateralTextureFilter::execute_c1(const std::uint8_t* const d_src, std::uint8_t* const d_dst,
                                            void* stream) {
    impl_->execute_c1(d_src, d_dst, stream);
}

// ------------------------------------------------------------ cuda_gradient
template <>
void cuda_gradient_impl<std::uint8_t>(const std::uint8_t* const d_src, float* const d_dst, const int width,
                                      const int height, const int src_ch) {
    VIP_REPORT(vip_gradient_u8(d_src, d_dst, width, height, src_ch, VIP_NUMERICS_CUDA, nullptr));
}

template <>
void cuda_gradient_impl<float>(const float* const d_src, float* const d_dst, const int width, const int height,
                               const int src_ch) {
    VIP_REPORT(vip_gradient_f32(d_src, d_dst, width, height, src_ch, VIP_NUMERICS_CUDA, nullptr));
}

// ------------------------------------------------------------ DeviceImage
template <typename ElemType>
class DeviceImage<ElemType>::Impl {
public:
    explicit Impl(const size_t len) : len_(len) {
        const int rc = vip_malloc(reinterpret_cast<void**>(&data_), len * sizeof(ElemType));
        if (rc) fail("DeviceImage", rc);
    }
    ~Impl() { vip_free(data_); }
    void upload(const ElemType* const data) { VIP_REPORT(vip_upload(data_, data, len_ * sizeof(ElemType))); }
    void download(ElemType* const data) { VIP_REPORT(vip_download(data, data_, len_ * sizeof(ElemType))); }
    void upload_async(const ElemType* const data, void* stream) {
        VIP_REPORT(vip_upload_async(data_, data, len_ * sizeof(ElemType), stream));
    }
    void download_async(ElemType* const data, void* stream) {
        VIP_REPORT(vip_download_async(data, data_, len_ * sizeof(ElemType), stream));
    }
    ElemType* get() { return data_; }

private:
    size_t len_;
    ElemType* data_ = nullptr;
};

template <typename ElemType>
DeviceImage<ElemType>::DeviceImage(const int width, const int height, const int channels)
    : impl_(new Impl((size_t)width * height * channels)) {}

template <typename ElemType>
DeviceImage<ElemType>::~DeviceImage() {
    delete impl_;
}

template <typename ElemType>
DeviceImage<ElemType>::DeviceImage(DeviceImage&& other) noexcept : impl_(other.impl_) {
    other.impl_ = nullptr;
}

template <typename ElemType>
DeviceImage<ElemType>& DeviceImage<ElemType>::operator=(DeviceImage&& other) noexcept {
    if (this != &other) {
        delete impl_;
        impl_ = other.impl_;
        other.impl_ = nullptr;
    }
    return *this;
}

template <typename ElemType>
void DeviceImage<ElemType>::upload(const ElemType* const data) {
    impl_->upload(data);
}

template <typename ElemType>
void DeviceImage<ElemType>::download(ElemType* const data) {
    impl_->download(data);
}

template <typename ElemType>
ElemType* DeviceImage<ElemType>::get() {
    return impl_->get();
}

template <typename ElemType>
void DeviceImage<ElemType>::upload_async(const ElemType* const data, void* stream) {
    impl_->upload_async(data, stream);
}

template <typename ElemType>
void DeviceImage<ElemType>::download_async(ElemType* const data, void* stream) {
    impl_->download_async(data, stream);
}

template class DeviceImage<std::uint8_t>;
template class DeviceImage<float>;
