// Self-guided f32 bilateral of 2 interleaved channels (vip_bilateral_f32c.hpp): every radius, separate multiply and add (CPP profile).
#include "vip_bilateral_f32c.hpp"

namespace vip {
template int launch_bilateral_f32c_unit<2, false>(int, const BilateralF32Args&, hipStream_t);
}  // namespace vip
