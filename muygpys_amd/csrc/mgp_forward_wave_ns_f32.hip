// The fp32 instantiations of the wave-sized forward with a length scale per neighbourhood (mgp_forward_wave_ns.h), in a
// translation unit of their own: compiled in parallel with mgp_forward_wave_ns.hip.
#include "mgp_forward_wave_ns.h"

namespace mgp {
template int launch_fwd_ns_dg<float, 32>(const FusedArgs&, const void*, hipStream_t);
template int launch_fwd_ns_dg<float, 64>(const FusedArgs&, const void*, hipStream_t);
}  // namespace mgp
