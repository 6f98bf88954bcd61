// The fp32 instantiations of the wave-sized backward of the general-smoothness Matern (mgp_backward_wave_gen.h), in a
// translation unit of their own: compiled in parallel with mgp_backward_wave_gen.hip.
#include "mgp_backward_wave_gen.h"

namespace mgp {
template int launch_bwd_gen_dg<float, 32>(const BackwardArgs&, void*, hipStream_t);
template int launch_bwd_gen_dg<float, 64>(const BackwardArgs&, void*, hipStream_t);
}  // namespace mgp
