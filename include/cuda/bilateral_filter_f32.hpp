// Self-guided bilateral filter of an f32 one-channel image (a depth map, an HDR luminance plane, a
// height field); no reference counterpart. Backed by the C ABI in include/vip.h
// (vip_bilateral_f32_*, libvip_hip.so, gfx950 HIP kernels), which holds the definition.
// Pointers are device pointers to dense width x height float images. value_range is the span of
// differences the 1024-bin range table covers (pass the image's max - min; larger differences take
// the weight at value_range). ksize odd, 1..31. The forms with `channels` (1..3) take dense images of
// that many interleaved floats per pixel; the range weight then comes from the L1 distance over the
// channels, value_range is the largest such distance the table covers (channels * (max - min) for
// OpenCV's behaviour), and ksize stops at 15 for 2 and 3 channels. The public call blocks until the GPU is done, like
// the other classes' public calls; the Impl's call (and the public one with a stream, a hipStream_t
// passed as void*, nullptr = default stream) enqueues and returns at once.
#ifndef VIP_CUDA_BILATERAL_FILTER_F32_HPP
#define VIP_CUDA_BILATERAL_FILTER_F32_HPP

#include <memory>

struct vip_bilateral_f32_s;

class CudaBilateralFilterF32 {
public:
    CudaBilateralFilterF32(const int width, const int height, const int ksize = 9, const float sigma_space = 10.f,
                           const float sigma_color = 30.f, const float value_range = 255.f);
    ~CudaBilateralFilterF32();

    void bilateral_filter(const float* const d_src, float* const d_dst) const;
    void bilateral_filter(const float* const d_src, float* const d_dst, void* stream) const;
    void bilateral_filter(const float* const d_src, const int channels, float* const d_dst) const;
    void bilateral_filter(const float* const d_src, const int channels, float* const d_dst, void* stream) const;
    // the range weight from a second one-channel float image of the same size, the guide
    // (vip_bilateral_f32_run_joint: a depth map under a luminance plane); value_range is then the
    // span of guide differences; d_guide == d_src gives bilateral_filter's result
    void joint_bilateral_filter(const float* const d_src, const float* const d_guide, float* const d_dst) const;
    void joint_bilateral_filter(const float* const d_src, const float* const d_guide, float* const d_dst,
                                void* stream) const;

    // no synchronisation
    class Impl {
    public:
        Impl(const int width, const int height, const int ksize, const float sigma_space, const float sigma_color,
             const float value_range);
        ~Impl();
        Impl(const Impl&) = delete;
        Impl& operator=(const Impl&) = delete;
        void bilateral_filter(const float* const d_src, float* const d_dst, void* stream = nullptr) const;
        void bilateral_filter(const float* const d_src, const int channels, float* const d_dst,
                              void* stream = nullptr) const;
        void joint_bilateral_filter(const float* const d_src, const float* const d_guide, float* const d_dst,
                                    void* stream = nullptr) const;

    private:
        const int width_;
        vip_bilateral_f32_s* handle_ = nullptr;
    };

protected:
    std::unique_ptr<Impl> impl_;
};

#endif  // VIP_CUDA_BILATERAL_FILTER_F32_HPP
