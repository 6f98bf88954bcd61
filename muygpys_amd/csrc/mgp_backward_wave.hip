// Backward pass on the phases of the wave kernel: the launcher by shape (mgp_backward_wave_kernel.h holds the
// kernel and states the maths).  The fp32 instantiations compile in translation units of their own
// (mgp_backward_wave_f32_np32.hip, mgp_backward_wave_f32_np64.hip), in parallel with this one.
#include "mgp_backward_wave_kernel.h"

namespace mgp {

extern template int launch_bwd_dg<float, 32>(const BackwardArgs&, hipStream_t);
extern template int launch_bwd_dg<float, 64>(const BackwardArgs&, hipStream_t);

// d <= 64 (fp32) / 16 (fp64), k + 2 <= 64 (fp32) / 32 (fp64); everything else: MGP_EUNSUPPORTED (the LDS workgroup kernel)
template <typename T>
int launch_backward_wave(const BackwardArgs& g, hipStream_t stream) {
  const int rows = g.f.k + 2;
  if ((g.f.ls_count != 1 && g.f.ls_count != g.f.d) || g.f.d > 16 * (16 / (int)sizeof(T)) || rows > 64) return MGP_EUNSUPPORTED;
  if (rows <= 32) return launch_bwd_dg<T, 32>(g, stream);
  if constexpr (sizeof(T) == 8) {
    // rows of at most 8 features (round 5; BASELINE config 4: k = 50, d = 8, whose L-BFGS-B gradient is this launch):
    // hyper-parameter gradients without the sweep at two waves per SIMD; with feature cotangents the sweep's 64-double
    // q row takes the whole register file (one wave per SIMD) -- still ahead of the LDS workgroup kernel
    if (g.f.d <= 8) return launch_bwd_np<T, 64, 4>(g, stream);
    return MGP_EUNSUPPORTED;
  } else {
    return launch_bwd_dg<T, 64>(g, stream);
  }
}

template int launch_backward_wave<float>(const BackwardArgs&, hipStream_t);
template int launch_backward_wave<double>(const BackwardArgs&, hipStream_t);

}  // namespace mgp
