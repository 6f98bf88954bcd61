// Hyper-parameter backward of the general-smoothness Matern (kernel_id MGP_KERNEL_MATERN_GEN, FusedArgs::smoothness) for
// every k with k + 2 <= kLargeMaxRows: hyper_backward_large_kernel (mgp_backward_large.hip: same slab, same phases out
// of mgp_backward_large.h, same launch rule) with the kernel function taken from the in-kernel evaluators of
// mgp_wave_common.h, and one more output: grad_nu (b), the partial with respect to the smoothness.
//
// What differs, per neighbourhood:
//   1. the squared distances always stay in the triangle; the last feature chunk copies them into the trapezoid, where
//      gen_covariance_phase (mgp_gen_launch.h) turns them into covariances as in fused_large_gen_kernel
//   4. strip-mined like gen_covariance_phase -- the evaluators end their node loop on a wave ballot, so every thread
//      makes the same number of calls; a strip = NT threads x 4 (fp32) / 2 (fp64) pairs, its map a function of k and
//      NT alone: per pair dk/dr and, NU, dk/dnu from one evaluator call, then liso += gK kp x (Isotropy),
//      Dst[p] = gK dk_dacc (Anisotropy), gnu += gK dk/dnu
// grad_nu is closed with block_sum_ordered like the isotropic length-scale sum: every sum runs in a fixed order, no
// floating-point atomic, a neighbourhood's outputs are the same bits wherever it is computed.
// LDS: the carve of mgp_backward_large.h, behind it the node table of the forward and the derivative table (2 + 2
// columns: 2 KiB in fp32, 8 KiB in fp64); the feature chunk is as wide as fits next to them, which it does for every
// k of the closed-form entry in both widths (backward_gen_large_max_nn_count = 1022).
#include "mgp_backward_large.h"
#include "mgp_gen_launch.h"

namespace mgp {

template <typename T, bool NU>
__global__ void __launch_bounds__(512) hyper_backward_gen_large_kernel(BackwardArgs g, T* gnu, T* workspace, int slab_elems,
                                                                        int factor_elems, GenLaunch gl) {
  constexpr int E = 16 / (int)sizeof(T);
  constexpr int PC = gen_pairs_per_call<T>();
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const FusedArgs& a = g.f;
  const int k_ = a.k, d = a.d, dc = a.dc;
  const BackwardLargeLds<T> s = backward_large_carve<T>(smem, k_, dc);
  T *av = s.av, *wv = s.wv;
  const T* tab = reinterpret_cast<const T*>(smem + gl.tab);
  const T* dtab = reinterpret_cast<const T*>(smem + gl.dtab);

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

  const IsoScale<T> iso = iso_scale<T, true>(a);
  const T post_scale = iso.post_scale, inv_l = iso.inv_l;
  gen_build_node_table<T>(reinterpret_cast<T*>(smem + gl.tab), a.smoothness, gl, tid);
  gen_build_deriv_node_table<T>(reinterpret_cast<T*>(smem + gl.dtab), a.smoothness, gl, tid);

  for (int64_t nb = blockIdx.x; nb < a.b; nb += gridDim.x) {
    __syncthreads();  // previous neighbourhood fully consumed (first round: the tables are written)
    int k = k_;
    asm volatile("" : "+s"(k));
    const int rows = k + 2;
    const int npairs = (k + 1) * k / 2;
    T* slab = workspace + (int64_t)blockIdx.x * slab_elems;
    const SlabRows<T> row{slab, k};
    T* Dst = slab + factor_elems;

    // ---- 1. squared distances (kept in Dst, copied into the trapezoid), covariances, nugget, the two tail rows ----
    fill_index_list(s.idx, a, nb, k, tid, NT);
    __syncthreads();
    pair_distances<T>(a, k, s.idx, s.X, s.XP, s.il, tid, NT, [&](int p, int r, int c, T acc, int d0, bool last) {
      if (d0 > 0) acc += Dst[p];
      Dst[p] = acc;
      if (last) row(r)[c] = acc;
    });
    // (each pair by the thread that wrote its distance: the strip map and pair_distances' both give pair p to p % NT)
    gen_covariance_phase<T>([&](int r, int c) { return row(r) + c; }, k, a.metric_id, post_scale, a.smoothness, gl, tab, tid, NT);
    fill_diagonal_and_rhs<T>(row, a, gmean, gyk, s.idx, nb, k, tid, NT);
    __syncthreads();

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
    if (gls || NU) {
      T liso = T(0), lnu = T(0);
      for (int p0 = 0; p0 < npairs; p0 += NT * PC) {  // (uniform trip count)
        T v[PC], x[PC], dn[PC];
        unsigned live = 0;
#pragma unroll
        for (int u = 0; u < PC; ++u) {
          const int p = p0 + u * NT + tid;
          v[u] = T(1);
          if (p < npairs) {
            v[u] = metric_arg<T>(Dst[p], a.metric_id, post_scale);
            live |= 1u << u;
          }
          x[u] = v[u];
          dn[u] = T(0);
        }
        gen_deriv_strip<T, NU>(v, dn, live, a.smoothness, gl, tab, dtab);
#pragma unroll
        for (int u = 0; u < PC; ++u) {
          if (!((live >> u) & 1u)) continue;
          const int p = p0 + u * NT + tid;
          int a_, c_;
          tri_decode(p, a_, c_);
          const T gK = pair_cotangent<T>(av, wv, a_, c_, k, gv, gm1, gyv);
          const T kp = v[u];
          if (gls) {
            if (aniso) Dst[p] = gK * dk_dacc<T>(x[u], kp, post_scale, l2);
            else liso += gK * kp * x[u];
          }
          if constexpr (NU) lnu += gK * dn[u];
        }
      }
      if (gls && !aniso) {
        const T total = block_sum_ordered<T>(liso, s.red, tid, NT);
        if (tid == 0) gls[nb] = -(l2 ? T(1) : T(2)) * inv_l * total;  // dx/dl = -x/l | -2x/l
      }
      if constexpr (NU) {
        const T total = block_sum_ordered<T>(lnu, s.red, tid, NT);
        if (tid == 0) gnu[nb] = total;
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

// the LDS of a launch: the closed-form backward's carve and both node tables behind it
template <typename T>
static size_t backward_gen_large_lds_bytes(int k, int dc) {
  return backward_large_lds_bytes<T>(k, dc) + gen_table_bytes(sizeof(T)) + gen_deriv_table_bytes(sizeof(T));
}
template <typename T>
static FeatureChunk backward_gen_large_chunk(int k, int d) {
  return feature_chunk(d, [&](int dc) { return backward_gen_large_lds_bytes<T>(k, dc); });
}

// the largest nn_count the entry serves: k + 2 <= kLargeMaxRows wherever the narrowest feature chunk fits LDS
int backward_gen_large_max_nn_count(int elem_size) {
  const auto fits = [&](int k) {
    if ((int64_t)k + 2 > kLargeMaxRows) return false;
    return elem_size == 8 ? backward_gen_large_chunk<double>(k, 1).fits : backward_gen_large_chunk<float>(k, 1).fits;
  };
  return largest_k(fits);
}

template <typename T>
int launch_hyper_backward_gen_large(const BackwardArgs& in, void* grad_nu, void* workspace, int64_t workspace_bytes,
                                    hipStream_t stream) {
  BackwardArgs g = in;
  const int64_t rows = (int64_t)g.f.k + 2;  // (64 bits: k near INT_MAX must not wrap past the limit)
  if (rows > kLargeMaxRows) return MGP_EUNSUPPORTED;
  const int k = g.f.k;
  const int64_t slab = backward_large_slab_bytes(sizeof(T), k);
  const FeatureChunk fc = backward_gen_large_chunk<T>(k, g.f.d);
  if (!fc.fits) return MGP_EUNSUPPORTED;
  g.f.dc = fc.dc;
  GenLaunch gl = gen_launch_constants(g.f.smoothness, sizeof(T) == 8);
  gl.tab = (int)backward_large_lds_bytes<T>(k, fc.dc);
  gl.dtab = gl.tab + (int)gen_table_bytes(sizeof(T));
  const bool nu = grad_nu != nullptr;
  // (one workgroup per slab, at most one per CU, at most b)
  const LaunchLabel label(g.f.b, k, g.f.d, g.f.R, "mgp::hyper_backward_gen_large_kernel<%s, %s>", sizeof(T) == 4 ? "float" : "double",
                          nu ? "true" : "false");
  const int threads = slab_block_threads((int)rows);
  const Capacity cap{kMaxPerCu, workspace_bytes / slab};
  const int slab_elems = (int)(slab / (int64_t)sizeof(T));
  const int factor_elems = (int)(large_slab_bytes(sizeof(T), k, 1) / (int64_t)sizeof(T));
  if (nu)
    return launch_capacity(&hyper_backward_gen_large_kernel<T, true>, threads, fc.lds, g.f.b, cap, stream, &label, g,
                           static_cast<T*>(grad_nu), static_cast<T*>(workspace), slab_elems, factor_elems, gl).status;
  return launch_capacity(&hyper_backward_gen_large_kernel<T, false>, threads, fc.lds, g.f.b, cap, stream, &label, g,
                         static_cast<T*>(nullptr), static_cast<T*>(workspace), slab_elems, factor_elems, gl).status;
}

template int launch_hyper_backward_gen_large<float>(const BackwardArgs&, void*, void*, int64_t, hipStream_t);
template int launch_hyper_backward_gen_large<double>(const BackwardArgs&, void*, void*, int64_t, hipStream_t);

}  // namespace mgp
