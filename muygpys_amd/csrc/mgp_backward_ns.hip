// Hyper-parameter backward of the LDS workgroup family with a length scale per neighbourhood (mgp_hyper_backward_ns_*,
// the rung behind the wave-sized kernel of mgp_backward_wave_ns.hip): backward_ns_body (mgp_backward_ns_kernel.h), the LDS backward restated with the scale read per neighbourhood, behind a second
// kernel argument, NsLaunch{ls_batch}.  (b, 1) and (b, d) scales, every noise mode, gyk given or not, any R in the
// posterior form.  The LDS carve, the feature chunk, the threads and the grid are those of launch_backward: with every
// row of ls_batch equal the launch returns the bits of mgp_posterior_backward_* on its LDS rung.
#include "mgp_backward_ns_kernel.h"

namespace mgp {

template <typename T>
__global__ __launch_bounds__(256) void ns_lds_backward_kernel(BackwardArgs g, NsLaunch n) { backward_ns_body<T>(g, n); }

template <typename T>
int launch_backward_ns(const BackwardArgs& in, const void* ls_batch, hipStream_t stream) {
  BackwardArgs g = in;
  if (g.f.kernel_id == MGP_KERNEL_MATERN_GEN) return MGP_EUNSUPPORTED;
  const FeatureChunk fc = feature_chunk(g.f.d, [&](int dc) { return backward_ns_lds_bytes<T>(g.f.k, dc); });
  if (!fc.fits) return MGP_EUNSUPPORTED;
  g.f.dc = fc.dc;
  g.f.length_scale = nullptr;  // (not read: the scales are the second argument's)
  const int threads = g.f.k + 2 <= 64 ? 64 : (g.f.k + 2 <= 128 ? 128 : 256);
  const LaunchLabel label(g.f.b, g.f.k, g.f.d, g.f.R, "mgp::ns_lds_backward_kernel<%s> [threads=%d,dc=%d]", sizeof(T) == 4 ? "float" : "double",
                          threads, fc.dc);
  return launch_capacity(&ns_lds_backward_kernel<T>, threads, fc.lds, g.f.b, Capacity{16}, stream, &label, g, NsLaunch{ls_batch}).status;
}

template int launch_backward_ns<float>(const BackwardArgs&, const void*, hipStream_t);
template int launch_backward_ns<double>(const BackwardArgs&, const void*, hipStream_t);

}  // namespace mgp
