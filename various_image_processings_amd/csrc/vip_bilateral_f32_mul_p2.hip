// Self-guided f32 bilateral (vip_bilateral_f32.hpp): the kernels of radius 14, separate multiply and add (CPP profile).
#include "vip_bilateral_f32.hpp"

namespace vip {

template <>
int launch_bilateral_f32_part<false, 2>(int radius, const BilateralF32Args& a, hipStream_t s) {
    return launch_bf32_part<false, 2>(radius, a, s);
}

}  // namespace vip
