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
  constexpr int E = 16 / (int)sizeof(T);
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const FusedArgs& a = g.f;
  const int k_ = a.k, d = a.d, dc = a.dc;
  const BackwardLargeLds<T> s = backward_large_carve<T>(smem, k_, dc);
  T *av = s.av, *wv = s.wv;

  const T* feat = static_cast<const T*>(a.feat_nn);
  const T* ls = static_cast<const T*>(a.length_scale);
  const T* gmean = static_cast<const T*>(g.grad_mean);
  const T* gvar = static_cast<const T*>(g.grad_var);
  const T* gyk = static_cast<const T*>(g.grad_yk);
  T* gls = static_cast<T*>(g.grad_ls);
  T* gnz = static_cast<T*>(g.grad_noise);
  const int tid = threadIdx.x, NT = blockDim.x;
  const bool aniso = a.ls_count > 1;
  const bool l2 = a.metric_id == MGP_METRIC_L2;
  const bool vec_ok = d % E == 0 && dc % E == 0 && (uintptr_t)feat % 16 == 0;
  // the distances are read again by the next feature chunk and by the length-scale cotangents: a grad_noise-only call
  // whose features fit one chunk stores none
  const bool keep_acc = gls != nullptr || d > dc;

  const IsoScale<T> iso = iso_scale<T, true>(a);
  const T post_scale = iso.post_scale, inv_l = iso.inv_l;

  for (int64_t nb = blockIdx.x; nb < a.b; nb += gridDim.x) {
    __syncthreads();  // previous neighbourhood fully consumed
    int k = k_;
    asm volatile("" : "+s"(k));
    const int rows = k + 2;
    const int npairs = (k + 1) * k / 2;
    T* slab = workspace + (int64_t)blockIdx.x * slab_elems;
    const SlabRows<T> row{slab, k};
    T* Dst = slab + factor_elems;

    // ---- 1. squared distances (kept in Dst), covariances, nugget, the two tail rows ----
    backward_large_assemble<T>(a, gmean, gyk, keep_acc, post_scale, nb, k, row, Dst, s, tid, NT);

    // ---- 2. factorisation; rows k, k + 1 then hold z = L^-1 c and zy = L^-1 yt ----
    const bool bad = factor_augmented_slab<T>(row, k, rows, s.Lb, tid, NT);
    if (bad) {  // uniform
      if (tid == 0 && a.info) atomicAdd(a.info, 1);
      continue;  // the partials of a non-SPD neighbourhood are left untouched
    }

    // ---- 3. back-substitution of both tail rows, in LDS ----
    backward_large_solve_tails<T>(row, k, av, wv, tid, NT);

    // ---- 4. cotangents: a = K^-1 c in av, w = K^-1 yt in wv ----
    const T gv = gvar ? gvar[nb] : T(0);
    const T gyv = gyk ? gyk[nb] : T(0);
    const T gm1 = gyk ? (gmean ? gmean[nb] : T(0)) : T(1);
    if (gls) {
      T liso = T(0);
      for (int p = tid; p < npairs; p += NT) {
        int a_, c_;
        tri_decode(p, a_, c_);
        const T gK = pair_cotangent<T>(av, wv, a_, c_, k, gv, gm1, gyv);
        const T x = metric_arg<T>(Dst[p], a.metric_id, post_scale);
        const T kp = kernel_deriv<T>(a.kernel_id, x);
        if (aniso) {
          Dst[p] = gK * dk_dacc<T>(x, kp, post_scale, l2);
        } else {
          liso += gK * kp * x;
        }
      }
      if (!aniso) {
        const T total = block_sum_ordered<T>(liso, s.red, tid, NT);
        if (tid == 0) gls[nb] = -(l2 ? T(1) : T(2)) * inv_l * total;  // dx/dl = -x/l | -2x/l
      }
    }
    if (gnz)
      for (int r = tid; r < k; r += NT) gnz[nb * k + r] = noise_cotangent<T>(av[r], wv[r], gv, gm1, gyv);
    if (!(gls && aniso)) continue;  // uniform

    // ---- 5. Anisotropy: grad_ls[c] = -2 / l_c^3 sum_pairs q_ij (x_ic - x_jc)^2 ----
    for (int d0 = 0; d0 < d; d0 += dc) {
      const int w = min(dc, d - d0);
      const int wp = (w + E - 1) / E * E;
      __syncthreads();  // q is in the triangle; the previous chunk's rows are consumed
      gather_tile_lds<T>(s.X, s.XP, feat, feat, s.idx, k, d, d0, w, wp, vec_ok, tid, NT);
      __syncthreads();
      backward_large_ls_chunk<T>(Dst, s.X, s.XP, s.red, ls + d0, gls + nb * (int64_t)a.ls_count + d0, w, wp, npairs, tid, NT);
    }
  }
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
