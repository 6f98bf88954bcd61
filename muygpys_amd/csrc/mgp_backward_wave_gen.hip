// Wave-sized hyper-parameter backward of the general-smoothness Matern: the launcher by shape (mgp_backward_wave_gen.h
// holds the kernel) and the fp64 instantiations; the fp32 ones compile in mgp_backward_wave_gen_f32.hip.
#include "mgp_backward_wave_gen.h"

namespace mgp {

extern template int launch_bwd_gen_dg<float, 32>(const BackwardArgs&, void*, hipStream_t);
extern template int launch_bwd_gen_dg<float, 64>(const BackwardArgs&, void*, hipStream_t);

// The shapes of launch_backward_wave_ns with either length-scale form: d <= 64 (fp32) / 16 (fp64, 8 at more than 32
// slots), k + 2 <= 64; everything else MGP_EUNSUPPORTED (the LDS workgroup backward, the slab).
template <typename T>
int launch_hyper_backward_gen_wave(const BackwardArgs& g, void* grad_nu, hipStream_t stream) {
  if (g.f.k > 62 || g.f.d > 16 * (16 / (int)sizeof(T))) return MGP_EUNSUPPORTED;  // (k near INT_MAX: no k + 2)
  if (g.f.k + 2 <= 32) return launch_bwd_gen_dg<T, 32>(g, grad_nu, stream);
  return launch_bwd_gen_dg<T, 64>(g, grad_nu, stream);
}

template int launch_hyper_backward_gen_wave<float>(const BackwardArgs&, void*, hipStream_t);
template int launch_hyper_backward_gen_wave<double>(const BackwardArgs&, void*, hipStream_t);

}  // namespace mgp
