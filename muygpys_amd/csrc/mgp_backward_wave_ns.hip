// Wave-sized backward with a length scale per neighbourhood: the launcher by shape (mgp_backward_wave_ns.h holds the
// kernel) and the fp64 instantiations; the fp32 ones compile in mgp_backward_wave_ns_f32.hip.
#include "mgp_backward_wave_ns.h"

namespace mgp {

extern template int launch_bwd_ns_dg<float, 32>(const BackwardArgs&, const void*, hipStream_t);
extern template int launch_bwd_ns_dg<float, 64>(const BackwardArgs&, const void*, hipStream_t);

// The shapes of launch_backward_wave, Isotropy alone and hyper-parameter partials alone: d <= 64 (fp32) / 16 (fp64, 8
// at more than 32 slots), k + 2 <= 64; everything else -- (b, d) scales included -- MGP_EUNSUPPORTED (the LDS workgroup
// backward).
template <typename T>
int launch_backward_wave_ns(const BackwardArgs& g, const void* ls_batch, hipStream_t stream) {
  const int rows = g.f.k + 2;
  if (g.f.ls_count != 1 || g.f.d > 16 * (16 / (int)sizeof(T)) || rows > 64) return MGP_EUNSUPPORTED;
  if (rows <= 32) return launch_bwd_ns_dg<T, 32>(g, ls_batch, stream);
  if constexpr (sizeof(T) == 8) {
    if (g.f.d <= 8) return launch_bwd_ns_np<T, 64, 4>(g, ls_batch, stream);
    return MGP_EUNSUPPORTED;
  } else {
    return launch_bwd_ns_dg<T, 64>(g, ls_batch, stream);
  }
}

template int launch_backward_wave_ns<float>(const BackwardArgs&, const void*, hipStream_t);
template int launch_backward_wave_ns<double>(const BackwardArgs&, const void*, hipStream_t);

}  // namespace mgp
