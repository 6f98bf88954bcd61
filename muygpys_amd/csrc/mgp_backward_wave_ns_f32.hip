// The fp32 instantiations of the wave-sized backward with a length scale per neighbourhood (mgp_backward_wave_ns.h),
// in a translation unit of their own: compiled in parallel with mgp_backward_wave_ns.hip.
#include "mgp_backward_wave_ns.h"

namespace mgp {
template int launch_bwd_ns_dg<float, 32>(const BackwardArgs&, const void*, hipStream_t);
template int launch_bwd_ns_dg<float, 64>(const BackwardArgs&, const void*, hipStream_t);
}  // namespace mgp
