// The whole vector-Jacobian product of the fused path for local systems beyond LDS (k + 2 <= kLargeMaxRows): every
// cotangent of mgp_backward.hip -- the feature tables, the neighbours' responses, the length scale(s), the noise
// diagonal -- on the backward slab and the phases of mgp_backward_large.h.  What the reference obtains from torch
// autograd when a deep-kernel model trains through MuyGPs_layer (torch/muygps_layer.py:129-164) at an nn_count whose
// two k x k triangles no longer fit LDS.  One workgroup per neighbourhood on a persistent grid, one backward slab per
// workgroup, as hyper_backward_large_kernel; two differences up to the factor: the query row comes from its own table
// (feat_q; row nb without batch_idx), and there is no y^T K^-1 y form.
//
// Per neighbourhood, phases 1 - 3 as there (assemble, factor_augmented_slab, both tail rows back-substituted in LDS), then
//   4. the response cotangents gm_r a_j (one atomic each); the cotangent q = gK dkappa/dacc of every pair into the
//      triangle -- under Isotropy too, with the scalar length scale folded into dkappa/dacc -- grad_noise, and the
//      isotropic length-scale sum in the hyper kernel's order
//   5. Anisotropy: the per-feature length-scale sums of a feature chunk, as there
//   6. the per-point sweep of the same staged chunk: x-bar_i = (2 / l_c^2) sum_j q_ij (x_ic - x_jc).  A thread owns one
//      point and eight features of it; lanes run along the points.  It reads the triangle from both ends: q(i, j),
//      j < i, is row i itself, walked 16 bytes at a time; q(j, i), j > i, lies at consecutive addresses for
//      consecutive i, so a wave's loads of one step are coalesced.  The rows x_j come from LDS as broadcasts.  The sum
//      of one (point, feature) is completed by its thread in ascending j and leaves as ONE atomic add: point k into
//      grad_feat_q, the others into grad_feat_nn.
// grad_ls and grad_noise are written by fixed-order sums alone and are the same bits whatever the placement; across
// neighbourhoods the three accumulated tables see one atomic per (row, column) and neighbourhood.  A neighbourhood with
// a bad pivot counts in *info before any of this: no atomic, no row written.
#include "mgp_backward_large.h"

namespace mgp {

// a 16-byte piece of a triangle row: rows start at any element
template <typename T> struct tri_vec;
template <> struct tri_vec<float> { typedef float type __attribute__((ext_vector_type(4), aligned(4))); };
template <> struct tri_vec<double> { typedef double type __attribute__((ext_vector_type(2), aligned(8))); };

// ---- 6. one feature chunk (rows staged in X, wp columns of which w are features): the points [i_lo, i_hi) ----
template <typename T>
__device__ __forceinline__ void posterior_backward_large_sweep(const T* Dst, const T* X, int XP, const int64_t* idx,
                                                               const T* ls_chunk, T* gq, T* gnn, int k, int d, int d0, int w,
                                                               int wp, int tid, int NT) {
  using V = typename lds_vec<T>::type;
  using VQ = typename tri_vec<T>::type;
  constexpr int E = 16 / (int)sizeof(T);
  constexpr int G = kBwdGroup / E;  // 16-byte pieces of a row per thread
  const int i_lo = gnn ? 0 : k, n_i = (gq ? k + 1 : k) - i_lo;
  const int groups = (wp + kBwdGroup - 1) / kBwdGroup;
  for (int t = tid; t < n_i * groups; t += NT) {
    const int grp = t / n_i, i = i_lo + (t - grp * n_i), c0 = grp * kBwdGroup;
    // (a piece at or beyond wp holds no feature: it is read -- the row has room for it -- and dropped below)
    V xi[G], s[G];
#pragma unroll
    for (int u = 0; u < G; ++u) {
      xi[u] = *reinterpret_cast<const V*>(X + i * XP + c0 + u * E);
      s[u] = V(0);
    }
    const T* xj = X + c0;
    // q(i, j), j < i: row i of the triangle
    const T* qi = Dst + i * (i - 1) / 2;
    int j = 0;
    for (; j + E <= i; j += E) {
      const VQ qv = *reinterpret_cast<const VQ*>(qi + j);
#pragma unroll
      for (int e = 0; e < E; ++e) {
#pragma unroll
        for (int u = 0; u < G; ++u) s[u] += qv[e] * (xi[u] - *reinterpret_cast<const V*>(xj + u * E));
        xj += XP;
      }
    }
    for (; j < i; ++j) {
      const T qv = qi[j];
#pragma unroll
      for (int u = 0; u < G; ++u) s[u] += qv * (xi[u] - *reinterpret_cast<const V*>(xj + u * E));
      xj += XP;
    }
    // q(j, i), j > i: column i, entry (j, i) at j (j - 1) / 2 + i
    xj += XP;
    const T* qc = Dst + (i + 1) * i / 2 + i;
#pragma unroll 2
    for (j = i + 1; j <= k; ++j) {
      const T qv = *qc;
      qc += j;
#pragma unroll
      for (int u = 0; u < G; ++u) s[u] += qv * (xi[u] - *reinterpret_cast<const V*>(xj + u * E));
      xj += XP;
    }
    T* out = (i < k ? gnn : gq) + idx[i] * (int64_t)d + d0 + c0;
#pragma unroll
    for (int u = 0; u < G; ++u)
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const int c = c0 + u * E + e;
        if (c >= w) continue;
        const T ilc = ls_chunk ? T(1) / ls_chunk[c] : T(1);  // (Isotropy: the scalar is inside q)
        unsafeAtomicAdd(out + u * E + e, T(2) * s[u][e] * ilc * ilc);
      }
  }
}

template <typename T>
__global__ void __launch_bounds__(512) posterior_backward_large_kernel(BackwardArgs g, T* workspace, int slab_elems, int factor_elems) {
  constexpr int E = 16 / (int)sizeof(T);
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const FusedArgs& a = g.f;
  const int k_ = a.k, d = a.d, R = a.R, dc = a.dc;
  const BackwardLargeLds<T> s = backward_large_carve<T>(smem, k_, dc);
  T *av = s.av, *wv = s.wv;

  const T* feat_q = static_cast<const T*>(a.feat_q);
  const T* feat_nn = static_cast<const T*>(a.feat_nn);
  const T* ls = static_cast<const T*>(a.length_scale);
  const T* gmean = static_cast<const T*>(g.grad_mean);
  const T* gvar = static_cast<const T*>(g.grad_var);
  T* gq = static_cast<T*>(g.grad_feat_q);
  T* gnn = static_cast<T*>(g.grad_feat_nn);
  T* gtg = static_cast<T*>(g.grad_targets);
  T* gls = static_cast<T*>(g.grad_ls);
  T* gnz = static_cast<T*>(g.grad_noise);
  const int tid = threadIdx.x, NT = blockDim.x;
  const bool aniso = a.ls_count > 1;
  const bool l2 = a.metric_id == MGP_METRIC_L2;
  const bool vec_ok = d % E == 0 && dc % E == 0 && ((uintptr_t)feat_q | (uintptr_t)feat_nn) % 16 == 0;
  const bool sweep = gq != nullptr || gnn != nullptr;
  const bool want_q = sweep || (gls && aniso);  // the pair cotangents go back into the triangle
  // the distances are read again by the next feature chunk and by every cotangent through the kernel function
  const bool keep_acc = gls != nullptr || sweep || d > dc;

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

    // ---- 1 - 3. the system, its factor, a = K^-1 c in av and w = K^-1 (Y gm) in wv ----
    backward_large_assemble<T>(a, gmean, static_cast<const T*>(nullptr), keep_acc, post_scale, nb, k, row, Dst, s, tid, NT);
    const bool bad = factor_augmented_slab<T>(row, k, rows, s.Lb, tid, NT);
    if (bad) {  // uniform
      if (tid == 0 && a.info) atomicAdd(a.info, 1);
      continue;  // a non-SPD neighbourhood issues no atomic and writes no row
    }
    backward_large_solve_tails<T>(row, k, av, wv, tid, NT);

    // ---- 4. cotangents ----
    const T gv = gvar ? gvar[nb] : T(0);
    if (gtg && gmean)
      for (int t = tid; t < k * R; t += NT) {
        const int c = t / R, r = t - c * R;
        unsafeAtomicAdd(gtg + s.idx[c] * (int64_t)R + r, gmean[nb * R + r] * av[c]);
      }
    if (gls || sweep) {
      T liso = T(0);
      for (int p = tid; p < npairs; p += NT) {
        int a_, c_;
        tri_decode(p, a_, c_);
        const T gK = pair_cotangent<T>(av, wv, a_, c_, k, gv, T(1), T(0));
        const T x = metric_arg<T>(Dst[p], a.metric_id, post_scale);
        const T kp = kernel_deriv<T>(a.kernel_id, x);
        if (want_q) Dst[p] = gK * dk_dacc<T>(x, kp, post_scale, l2);
        liso += gK * kp * x;
      }
      if (gls && !aniso) {
        const T total = block_sum_ordered<T>(liso, s.red, tid, NT);
        if (tid == 0) gls[nb] = -(l2 ? T(1) : T(2)) * inv_l * total;  // dx/dl = -x/l | -2x/l
      }
    }
    if (gnz)
      for (int r = tid; r < k; r += NT) gnz[nb * k + r] = noise_cotangent<T>(av[r], wv[r], gv);
    if (!want_q) continue;  // uniform

    // ---- 5, 6. per feature chunk: the per-feature length-scale sums, the per-point sweep ----
    for (int d0 = 0; d0 < d; d0 += dc) {
      const int w = min(dc, d - d0);
      const int wp = (w + E - 1) / E * E;
      __syncthreads();  // q is in the triangle; the previous chunk's rows are consumed
      gather_tile_lds<T>(s.X, s.XP, feat_q, feat_nn, s.idx, k, d, d0, w, wp, vec_ok, tid, NT);
      __syncthreads();
      if (gls && aniso)
        backward_large_ls_chunk<T>(Dst, s.X, s.XP, s.red, ls + d0, gls + nb * (int64_t)a.ls_count + d0, w, wp, npairs, tid, NT);
      if (sweep)
        posterior_backward_large_sweep<T>(Dst, s.X, s.XP, s.idx, aniso ? ls + d0 : nullptr, gq, gnn, k, d, d0, w, wp, tid, NT);
    }
  }
}

template <typename T>
int launch_posterior_backward_large(const BackwardArgs& in, void* workspace, int64_t workspace_bytes, hipStream_t stream) {
  BackwardArgs g = in;
  const int64_t rows = (int64_t)g.f.k + 2;  // (64 bits: k near INT_MAX must not wrap past the limit)
  if (rows > kLargeMaxRows || g.f.kernel_id == MGP_KERNEL_MATERN_GEN) return MGP_EUNSUPPORTED;
  const int k = g.f.k;
  const int64_t slab = backward_large_slab_bytes(sizeof(T), k);
  const FeatureChunk fc = backward_large_chunk<T>(k, g.f.d);
  if (!fc.fits) return MGP_EUNSUPPORTED;
  g.f.dc = fc.dc;
  // (one workgroup per slab, at most one per CU, at most b)
  const LaunchLabel label(g.f.b, k, g.f.d, g.f.R, "mgp::posterior_backward_large_kernel<%s>", sizeof(T) == 4 ? "float" : "double");
  return launch_capacity(&posterior_backward_large_kernel<T>, slab_block_threads((int)rows), fc.lds, g.f.b, Capacity{kMaxPerCu, workspace_bytes / slab},
                         stream, &label, g, static_cast<T*>(workspace), (int)(slab / (int64_t)sizeof(T)),
                         (int)(large_slab_bytes(sizeof(T), k, 1) / (int64_t)sizeof(T))).status;
}

template int launch_posterior_backward_large<float>(const BackwardArgs&, void*, int64_t, hipStream_t);
template int launch_posterior_backward_large<double>(const BackwardArgs&, void*, int64_t, hipStream_t);

}  // namespace mgp
