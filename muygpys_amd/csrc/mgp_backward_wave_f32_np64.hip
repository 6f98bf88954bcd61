// The fp32 instantiations of the wave backward kernel with 64 slots per neighbourhood (a translation unit of
// their own so that they compile in parallel with the rest of mgp_backward_wave.hip).
#include "mgp_backward_wave_kernel.h"

namespace mgp {
template int launch_bwd_dg<float, 64>(const BackwardArgs&, hipStream_t);
}  // namespace mgp
