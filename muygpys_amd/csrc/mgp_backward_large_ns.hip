// Hyper-parameter backward on the slab factor with a length scale per neighbourhood (mgp_hyper_backward_ns_large_*):
// the NS instantiation of hyper_backward_large_body (mgp_backward_large.h) behind a last kernel argument,
// NsLaunch{ls_batch}.  (b, 1) and (b, d) scales, up to nn_count 1022 on the workspace rule of
// mgp_hyper_backward_large_*; the slab, the LDS carve, the threads and the grid are the scalar launch's: with every row
// of ls_batch equal the launch returns its bits.
#include "mgp_backward_large.h"

namespace mgp {

template <typename T>
__global__ void __launch_bounds__(512) ns_slab_backward_kernel(BackwardArgs g, T* workspace, int slab_elems, int factor_elems, NsLaunch n) {
  hyper_backward_large_body<T, true>(g, workspace, slab_elems, factor_elems, n);
}

template <typename T>
int launch_hyper_backward_large_ns(const BackwardArgs& in, const void* ls_batch, void* workspace, int64_t workspace_bytes, hipStream_t stream) {
  BackwardArgs g = in;
  const int64_t rows = (int64_t)g.f.k + 2;  // (64 bits: k near INT_MAX must not wrap past the limit)
  if (rows > kLargeMaxRows || g.f.kernel_id == MGP_KERNEL_MATERN_GEN) return MGP_EUNSUPPORTED;
  const int k = g.f.k;
  const int64_t slab = backward_large_slab_bytes(sizeof(T), k);
  const FeatureChunk fc = backward_large_chunk<T>(k, g.f.d);
  if (!fc.fits) return MGP_EUNSUPPORTED;
  g.f.dc = fc.dc;
  g.f.length_scale = nullptr;  // (not read: the scales are the last argument's)
  const LaunchLabel label(g.f.b, k, g.f.d, g.f.R, "mgp::ns_slab_backward_kernel<%s>", sizeof(T) == 4 ? "float" : "double");
  return launch_capacity(&ns_slab_backward_kernel<T>, slab_block_threads((int)rows), fc.lds, g.f.b, Capacity{kMaxPerCu, workspace_bytes / slab},
                         stream, &label, g, static_cast<T*>(workspace), (int)(slab / (int64_t)sizeof(T)),
                         (int)(large_slab_bytes(sizeof(T), k, 1) / (int64_t)sizeof(T)), NsLaunch{ls_batch}).status;
}

template int launch_hyper_backward_large_ns<float>(const BackwardArgs&, const void*, void*, int64_t, hipStream_t);
template int launch_hyper_backward_large_ns<double>(const BackwardArgs&, const void*, void*, int64_t, hipStream_t);

}  // namespace mgp
