// Joint bilateral upsampling of 4 interleaved f32 channels (RGBA): the 4-channel kernels of
// vip_upsample_f32c.hpp, every radius, scale, guide form and arithmetic.
#include "vip_upsample_f32c.hpp"

namespace vip {
template int launch_upsample_f32c_channels<4>(int, int, int, bool, const UpsampleArgs&, hipStream_t);
}  // namespace vip
