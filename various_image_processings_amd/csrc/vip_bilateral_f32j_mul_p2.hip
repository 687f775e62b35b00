// f32 joint bilateral under an f32 guide (vip_bilateral_f32j.hpp): the kernels of radius 14, separate multiply and add (CPP profile).
#include "vip_bilateral_f32j.hpp"

namespace vip {

template <>
int launch_bilateral_f32_joint_part<false, 2>(int radius, const BilateralF32Args& a, hipStream_t s) {
    return launch_bf32j_part<false, 2>(radius, a, s);
}

}  // namespace vip
