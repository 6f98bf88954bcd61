// The fp32 instantiations of the wave backward kernel with 32 slots per neighbourhood (a translation unit of
// their own so that they compile in parallel with the rest of mgp_backward_wave.hip).
#include "mgp_backward_wave_kernel.h"

namespace mgp {
template int launch_bwd_dg<float, 32>(const BackwardArgs&, hipStream_t);
}  // namespace mgp
