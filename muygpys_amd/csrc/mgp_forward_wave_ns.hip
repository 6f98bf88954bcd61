// Wave-sized forward with a length scale per neighbourhood: the launcher by shape (mgp_forward_wave_ns.h holds the
// kernel) and the fp64 instantiations; the fp32 ones compile in mgp_forward_wave_ns_f32.hip.
#include "mgp_forward_wave_ns.h"

namespace mgp {

extern template int launch_fwd_ns_dg<float, 32>(const FusedArgs&, const void*, hipStream_t);
extern template int launch_fwd_ns_dg<float, 64>(const FusedArgs&, const void*, hipStream_t);

// The shapes of launch_backward_wave_ns, so that wherever the gradient is wave-sized the forward is too: Isotropy,
// k + 1 + R <= 64 slots, d <= 64 (fp32) / 16 (fp64, 8 at more than 32 slots); everything else -- (b, d) scales
// included -- MGP_EUNSUPPORTED (the LDS workgroup kernel).  Decided before any HIP call.
template <typename T>
int launch_forward_wave_ns(const FusedArgs& a, const void* ls_batch, hipStream_t stream) {
  const int64_t rows = (int64_t)a.k + 1 + a.R;
  constexpr int DMAX = sizeof(T) == 4 ? 64 : 16;
  if (a.ls_count != 1 || a.d > DMAX || rows > 64) return MGP_EUNSUPPORTED;
  if (rows <= 32) return launch_fwd_ns_dg<T, 32>(a, ls_batch, stream);
  if constexpr (sizeof(T) == 8) {
    if (a.d <= 8) return launch_fwd_ns_np<T, 64, 4>(a, ls_batch, stream);
    return MGP_EUNSUPPORTED;
  } else {
    return launch_fwd_ns_dg<T, 64>(a, ls_batch, stream);
  }
}

template int launch_forward_wave_ns<float>(const FusedArgs&, const void*, hipStream_t);
template int launch_forward_wave_ns<double>(const FusedArgs&, const void*, hipStream_t);

}  // namespace mgp
