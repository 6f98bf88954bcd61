// Hyper-parameter backward for local systems beyond LDS (k + 2 <= kLargeMaxRows): the length-scale and noise partials
// of mgp_backward.hip -- same formulas, no feature or response cotangents -- on the slab and the blocked factor of
// mgp_large_factor.h.  One workgroup per neighbourhood on a persistent grid, one backward slab of a caller-provided
// workspace per workgroup; the only cross-workgroup atomic is the one on *info.
//
// Backward slab: [factor trapezoid of k + 2 rows: K + diag(eps), c, yt][strict lower triangle of the (k+1)-point set,
// row after row: acc of every pair, later its cotangent q], each region in whole 256-byte lines.  The query is the
// training row batch_idx[nb]: one table serves both sides, as in LOOCV.
//
// Per neighbourhood (the phases are in mgp_backward_large.h, shared with the whole vector-Jacobian product of
// mgp_backward_large_full.hip):
//   1. assemble with the front end of fused_large_kernel (mgp_assemble.h: feature chunks of dc columns through LDS);
//      the squared distances accumulate in the triangle and stay there, the last chunk writes the covariances into the
//      trapezoid.  Two tail rows whatever R is: c, and ONE combined right-hand side yt = y (LOOCV form) or Y gm
//   2. factor_augmented_slab, unchanged
//   3. back-substitution L^T [a w] = [z zy] by the scheme of solve_large_kernel's coefficient output (column by column
//      from the last, row j of L read contiguously, the inverse pivot on its diagonal) with both tail rows in LDS: the
//      chain of k dependent steps runs through LDS, and row j - 1 of L is on its way from the slab while step j runs
//   4. cotangent of every pair (the formulas of mgp_backward.hip, their shared pieces in mgp_assemble.h), grad_noise,
//      the isotropic length-scale sum
//   5. Anisotropy: the triangle now holds q = gK dkappa/dacc; per feature chunk the rows are staged in LDS again and
//      eight features at a time are summed over all pairs
// Every sum is per-thread partials in a fixed pair order -> wave_sum -> the waves' totals in wave order through LDS:
// no floating-point atomic, so what a neighbourhood returns depends on nothing but its own inputs (the block size is
// a function of k alone).
#include "mgp_backward_large.h"

namespace mgp {

template <typename T>
__global__ void __launch_bounds__(512) hyper_backward_large_kernel(BackwardArgs g, T* workspace, int slab_elems, int factor_elems) {
  hyper_backward_large_body<T, false>(g, workspace, slab_elems, factor_elems, NsLaunch{});
}

// the factor trapezoid with two tail rows, then the triangle of the (k+1)-point set: whole 256-byte lines each
int64_t backward_large_slab_bytes(int elem_size, int k) {
  const int64_t factor = large_slab_bytes(elem_size, k, 1);
  const int64_t tri = (int64_t)k * ((int64_t)k + 1) / 2;
  if (factor == INT64_MAX || tri > (INT64_MAX - factor - 255) / elem_size) return INT64_MAX;
  return factor + (tri * elem_size + 255) / 256 * 256;
}

int64_t backward_large_workspace_bytes(int elem_size, int k, int64_t b) {
  const int64_t slab = backward_large_slab_bytes(elem_size, k), n = slab_count(b);
  return n * slab > kMaxWorkspace ? kMaxWorkspace : n * slab;
}

template <typename T>
int launch_hyper_backward_large(const BackwardArgs& in, void* workspace, int64_t workspace_bytes, hipStream_t stream) {
  BackwardArgs g = in;
  const int64_t rows = (int64_t)g.f.k + 2;  // (64 bits: k near INT_MAX must not wrap past the limit)
  if (rows > kLargeMaxRows || g.f.kernel_id == MGP_KERNEL_MATERN_GEN) return MGP_EUNSUPPORTED;
  const int k = g.f.k;
  const int64_t slab = backward_large_slab_bytes(sizeof(T), k);
  const FeatureChunk fc = backward_large_chunk<T>(k, g.f.d);
  if (!fc.fits) return MGP_EUNSUPPORTED;
  g.f.dc = fc.dc;
  // (one workgroup per slab, at most one per CU, at most b)
  const LaunchLabel label(g.f.b, k, g.f.d, g.f.R, "mgp::hyper_backward_large_kernel<%s>", sizeof(T) == 4 ? "float" : "double");
  return launch_capacity(&hyper_backward_large_kernel<T>, slab_block_threads((int)rows), fc.lds, g.f.b, Capacity{kMaxPerCu, workspace_bytes / slab},
                         stream, &label, g, static_cast<T*>(workspace), (int)(slab / (int64_t)sizeof(T)),
                         (int)(large_slab_bytes(sizeof(T), k, 1) / (int64_t)sizeof(T))).status;
}

template int launch_hyper_backward_large<float>(const BackwardArgs&, void*, int64_t, hipStream_t);
template int launch_hyper_backward_large<double>(const BackwardArgs&, void*, int64_t, hipStream_t);

}  // namespace mgp
