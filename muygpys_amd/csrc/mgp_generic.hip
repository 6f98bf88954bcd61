// Generic (any nn_count that fits LDS) kernels of the local-GP hot path:
//   * fused gather -> distances -> kernel -> nugget -> factor -> mean/var/yKinvy
//   * the same factorisation on a materialised Kin (API parity: S1/S2/S3 + fast precompute)
// One workgroup owns one neighbourhood at a time; its whole local system lives in LDS
// (see mgp_lds_factor.h); the assembly of the system is the one of mgp_assemble.h, shared with mgp_large.hip and the
// backward kernels.  The specialised register-resident kernels in mgp_fused_wave.hip
// take over for the shapes they cover; this file is the path for everything else.
#include "mgp_args.h"
#include "mgp_assemble.h"
#include "mgp_gen_launch.h"
#include "mgp_large_factor.h"
#include "mgp_launch.h"
#include "mgp_lds_factor.h"

namespace mgp {

// dynamic LDS carve (every array 16-byte aligned):
// [idx: (k+2 & ~1) int64][S: rows*SP T][X: (k+1)*XP T][il: dc T][piv: k T][flag]
// GEN (the general-smoothness Matern, a.smoothness): + [node table: 2 MGP_GEN_NODES float / 2 MGP_GEN_NODES64 double]
// at byte g.tab, behind everything else; the closed-form instantiations reserve and read nothing of `g`.
// COEFFS (a.coeffs set, no query, no mean / var / yKinvy: the fast-mean precompute): the back-substitution behind the
// factorisation, K^-1 y_r into a.coeffs (b, k, R).  An instantiation of its own, so that the kernels of every other
// entry are compiled from what they always were.
// NS (per-neighbourhood length scales, `n`: mgp_assemble.h): the scale(s) of neighbourhood nb come from row nb of
// n.ls_batch, handed to the shared front end in the place of a.length_scale (iso_scale_at, pair_distances_at);
// closed-form kernels only.  An instantiation of its own again; `ls` is a.length_scale everywhere else.
template <typename T, bool GEN, bool COEFFS = false, bool NS = false>
__device__ __forceinline__ void fused_generic_body(const FusedArgs& a, const GenLaunch& g, const NsLaunch& n = NsLaunch{}) {
  static_assert(!NS || (!GEN && !COEFFS), "per-neighbourhood scales: the closed-form posterior alone");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int k = a.k, R = a.R, dc = a.dc;
  const int rows = k + 1 + R;
  const int SP = lds_row_stride<T>(k);
  const int XP = tile_row_stride<T>(dc);
  int64_t* idx = reinterpret_cast<int64_t*>(smem);
  T* S = reinterpret_cast<T*>(idx + ((k + 2) & ~1));
  T* X = S + rows * SP;
  T* il = X + (k + 1) * XP;
  T* piv = il + dc;
  int* flag = reinterpret_cast<int*>(piv + k);
  const StridedRows<T> row{S, SP};

  const int tid = threadIdx.x, NT = blockDim.x;
  T post_scale = T(1);
  if constexpr (!NS) post_scale = iso_scale<T, false>(a).post_scale;
  const T* ls = static_cast<const T*>(a.length_scale);  // (NS: row nb of n.ls_batch, per neighbourhood)
  if constexpr (GEN) gen_build_node_table<T>(reinterpret_cast<T*>(smem + g.tab), a.smoothness, g, tid);

  for (int64_t nb = blockIdx.x; nb < a.b; nb += gridDim.x) {
    __syncthreads();  // previous neighbourhood fully consumed
    if constexpr (COEFFS) fill_index_list_no_query(idx, a, nb, k, tid, NT);
    else fill_index_list(idx, a, nb, k, tid, NT);
    __syncthreads();
    if constexpr (NS) {
      // a scale that is not finite and > 0: NaN outputs and one count in info, like a non-positive pivot; uniform
      // across the workgroup, and the other neighbourhoods of the launch see nothing of it
      bool bad_scale;
      ls = ns_select_scales<T>(a, n, nb, &bad_scale);
      if (bad_scale) {
        ns_refuse_neighbourhood<T>(a, nb, R, tid, NT);
        continue;
      }
      post_scale = iso_scale_at<T, false>(a, ls).post_scale;
    }

    // ---- assemble: squared distances summed over the feature chunks in S, covariances in place in a second pass, the
    // nugget on the diagonal, the responses into the tail rows ----
    pair_distances_at<T>(a, ls, k, idx, X, XP, il, tid, NT, [&](int, int r, int c, T acc, int d0, bool) {
      T* dst = row(r) + c;
      *dst = d0 == 0 ? acc : *dst + acc;
    });
    if constexpr (GEN) {
      // (whole strips of NT x 4 / NT x 2 pairs, every thread in every evaluator call: mgp_gen_launch.h)
      gen_covariance_phase<T>([&](int r, int c) { return row(r) + c; }, k, a.metric_id, post_scale, a.smoothness, g,
                              reinterpret_cast<const T*>(smem + g.tab), tid, NT);
    } else {
      for (int p = tid; p < (k + 1) * k / 2; p += NT) {
        int r, c;
        tri_decode(p, r, c);
        T* dst = row(r) + c;
        *dst = kernel_eval<T>(a.kernel_id, metric_arg<T>(*dst, a.metric_id, post_scale));
      }
    }
    // (responses first: the two loops are independent, and fused_generic_kernel<float> at k = 192, d = 40 measured 3 %
    // faster in this order than in the other -- the same loops elsewhere, placed differently)
    fill_responses<T>(row, a, idx, nb, k, R, tid, NT);
    fill_diagonal<T>(row, a, idx, nb, k, tid, NT);
    __syncthreads();

    // ---- factor, finish ----
    const bool bad = factor_augmented_rows<T>(row, k, rows, piv, flag, tid, NT);
    T* mean = static_cast<T*>(a.mean);
    T* var = static_cast<T*>(a.var);
    T* yk = static_cast<T*>(a.ykinvy);
    emit_outputs<T>(row, k, R, T(1), bad, true, mean ? mean + nb * R : nullptr, var ? var + nb : nullptr,
                    yk ? yk + nb * R : nullptr, tid);
    if constexpr (COEFFS) {
      // all R responses at once, column by column across the workgroup (piv: the inverse pivots)
      if (a.coeffs)
        back_substitute_columns<T>(row, k, R, [&](int j) { return piv[j]; }, bad, static_cast<T*>(a.coeffs) + nb * (int64_t)k * R, tid, NT);
    }
    if (bad && tid == 0 && a.info) atomicAdd(a.info, 1);
  }
}

// the closed-form kernels, the same with the coefficient output, and the general-smoothness Matern under a name of its
// own (its constants: an argument of its own)
template <typename T>
__global__ void fused_generic_kernel(FusedArgs a) { fused_generic_body<T, false>(a, GenLaunch{}); }
template <typename T>
__global__ void fused_generic_coeffs_kernel(FusedArgs a) { fused_generic_body<T, false, true>(a, GenLaunch{}); }
template <typename T>
__global__ void fused_generic_gen_kernel(FusedArgs a, GenLaunch g) { fused_generic_body<T, true>(a, g); }
// ... and its coefficient output (mgp_fast_coefficients_gen_*): GEN x COEFFS, an instantiation of its own as well
template <typename T>
__global__ void fused_generic_gen_coeffs_kernel(FusedArgs a, GenLaunch g) { fused_generic_body<T, true, true>(a, g); }
// ... and the closed-form kernels with a length scale per neighbourhood (mgp_posterior_ns_generic_*)
template <typename T>
__global__ void fused_generic_ns_kernel(FusedArgs a, NsLaunch n) { fused_generic_body<T, false, false, true>(a, GenLaunch{}, n); }

// LDS carve: [S: rows*SP T][piv: k T][flag]
template <typename T>
__global__ void solve_generic_kernel(SolveArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int k = a.k, R = a.R;
  const int rows = k + 1 + R;
  const int SP = lds_row_stride<T>(k);
  T* S = reinterpret_cast<T*>(smem);
  T* piv = S + rows * SP;
  int* flag = reinterpret_cast<int*>(piv + k);
  const T* Kin = static_cast<const T*>(a.Kin);
  const T* Kcross = static_cast<const T*>(a.Kcross);
  const T* Y = static_cast<const T*>(a.Y);
  const int tid = threadIdx.x, NT = blockDim.x;

  for (int64_t nb = blockIdx.x; nb < a.b; nb += gridDim.x) {
    __syncthreads();
    const T* Kb = Kin + nb * (int64_t)k * k;
    for (int t = tid; t < k * k; t += NT) {
      const int i = t / k, j = t - i * k;
      if (j <= i) S[i * SP + j] = Kb[t];  // lower triangle, as LAPACK 'L' would read it
    }
    for (int c = tid; c < k; c += NT) S[k * SP + c] = Kcross ? Kcross[nb * k + c] : T(0);
    for (int t = tid; t < k * R; t += NT) {
      const int c = t / R, r = t - c * R;
      S[(k + 1 + r) * SP + c] = Y[(nb * k + c) * (int64_t)R + r];
    }
    __syncthreads();
    const bool bad = factor_augmented_lds<T>(S, SP, k, rows, piv, flag, tid, NT);
    T* mean = static_cast<T*>(a.mean);
    T* var = static_cast<T*>(a.var);
    T* yk = static_cast<T*>(a.ykinvy);
    emit_outputs<T>(StridedRows<T>{S, SP}, k, R, (T)a.kout, bad, Kcross != nullptr, mean ? mean + nb * R : nullptr,
                    var ? var + nb : nullptr, yk ? yk + nb * R : nullptr, tid);
    if (a.coeffs) {
      // back-substitution L^T x = (L^-1 y_r), one response per thread, in place in row k+1+r
      T* co = static_cast<T*>(a.coeffs) + nb * (int64_t)k * R;
      __syncthreads();
      for (int r = tid; r < R; r += NT) {
        T* x = S + (k + 1 + r) * SP;
        for (int j = k - 1; j >= 0; --j) {
          T s = x[j];
          for (int m = j + 1; m < k; ++m) s -= S[m * SP + j] * x[m];
          x[j] = s * piv[j];
        }
        for (int j = 0; j < k; ++j) co[j * (int64_t)R + r] = bad ? num<T>::nan() : x[j];
      }
    }
    if (bad && tid == 0 && a.info) atomicAdd(a.info, 1);
  }
}

template <typename T>
static size_t fused_lds_bytes(int k, int R, int dc) {
  const int rows = k + 1 + R, SP = lds_row_stride<T>(k);
  size_t n = (size_t)((k + 2) & ~1) * sizeof(int64_t);
  n += ((size_t)rows * SP + (size_t)(k + 1) * tile_row_stride<T>(dc) + dc + k) * sizeof(T) + 16;
  return (n + 15) & ~(size_t)15;
}
template <typename T>
static size_t solve_lds_bytes(int k, int R) {
  const int rows = k + 1 + R, SP = lds_row_stride<T>(k);
  size_t n = ((size_t)rows * SP + k) * sizeof(T) + 16;
  return (n + 15) & ~(size_t)15;
}

// (at most 16 workgroups per CU: mgp_launch.h, capacity_grid)
// GEN: the general-smoothness Matern (a.smoothness); the LDS rule is "fits with the node table", which lies behind what
// the closed-form launch of the same shape and chunk takes
template <typename T, bool GEN>
static int launch_fused_generic_impl(const FusedArgs& in, hipStream_t stream) {
  FusedArgs a = in;
  if ((int64_t)a.k + 1 + a.R > kLargeMaxRows && GEN) return MGP_EUNSUPPORTED;  // (64 bits: k or R near INT_MAX)
  const size_t table = GEN ? gen_table_bytes(sizeof(T)) : 0;
  // feature chunk: as wide as fits next to the factor (bounded so small problems stay small)
  const FeatureChunk fc = feature_chunk(a.d, [&](int dc) { return fused_lds_bytes<T>(a.k, a.R, dc) + table; });
  if (!fc.fits) return MGP_EUNSUPPORTED;
  a.dc = fc.dc;
  GenLaunch g{};
  if (GEN) {
    g = gen_launch_constants(a.smoothness, sizeof(T) == 8);
    g.tab = (int)(fc.lds - table);
  }
  const LaunchLabel label(a.b, a.k, a.d, a.R, "mgp::fused_generic%s%s_kernel<%s>", GEN ? "_gen" : "", a.coeffs ? "_coeffs" : "", sizeof(T) == 4 ? "float" : "double");
  const int threads = lds_factor_threads(a.k + 1 + a.R);
  if constexpr (GEN) {
    if (a.coeffs) return launch_capacity(&fused_generic_gen_coeffs_kernel<T>, threads, fc.lds, a.b, Capacity{16}, stream, &label, a, g).status;
    return launch_capacity(&fused_generic_gen_kernel<T>, threads, fc.lds, a.b, Capacity{16}, stream, &label, a, g).status;
  }
  else if (a.coeffs) return launch_capacity(&fused_generic_coeffs_kernel<T>, threads, fc.lds, a.b, Capacity{16}, stream, &label, a).status;
  else return launch_capacity(&fused_generic_kernel<T>, threads, fc.lds, a.b, Capacity{16}, stream, &label, a).status;
}
template <typename T>
int launch_fused_generic(const FusedArgs& a, hipStream_t stream) { return launch_fused_generic_impl<T, false>(a, stream); }
template <typename T>
int launch_fused_generic_gen(const FusedArgs& a, hipStream_t stream) { return launch_fused_generic_impl<T, true>(a, stream); }

// per-neighbourhood length scales: the LDS carve, the feature chunk, the threads and the grid of the scalar launch
template <typename T>
int launch_fused_generic_ns(const FusedArgs& in, const void* ls_batch, hipStream_t stream) {
  FusedArgs a = in;
  if (a.kernel_id == MGP_KERNEL_MATERN_GEN || a.coeffs) return MGP_EUNSUPPORTED;
  const FeatureChunk fc = feature_chunk(a.d, [&](int dc) { return fused_lds_bytes<T>(a.k, a.R, dc); });
  if (!fc.fits) return MGP_EUNSUPPORTED;
  a.dc = fc.dc;
  a.length_scale = nullptr;  // (not read: the scales are the second argument's)
  const LaunchLabel label(a.b, a.k, a.d, a.R, "mgp::fused_generic_ns_kernel<%s>", sizeof(T) == 4 ? "float" : "double");
  return launch_capacity(&fused_generic_ns_kernel<T>, lds_factor_threads(a.k + 1 + a.R), fc.lds, a.b, Capacity{16}, stream, &label, a,
                         NsLaunch{ls_batch}).status;
}

template <typename T>
int launch_solve_generic(const SolveArgs& a, hipStream_t stream) {
  const size_t lds = solve_lds_bytes<T>(a.k, a.R);
  if (lds > kCuLdsBytes) return MGP_EUNSUPPORTED;
  return launch_capacity(&solve_generic_kernel<T>, lds_factor_threads(a.k + 1 + a.R), lds, a.b, Capacity{16}, stream, nullptr, a).status;
}

template int launch_fused_generic<float>(const FusedArgs&, hipStream_t);
template int launch_fused_generic<double>(const FusedArgs&, hipStream_t);
template int launch_fused_generic_gen<float>(const FusedArgs&, hipStream_t);
template int launch_fused_generic_gen<double>(const FusedArgs&, hipStream_t);
template int launch_fused_generic_ns<float>(const FusedArgs&, const void*, hipStream_t);
template int launch_fused_generic_ns<double>(const FusedArgs&, const void*, hipStream_t);
template int launch_solve_generic<float>(const SolveArgs&, hipStream_t);
template int launch_solve_generic<double>(const SolveArgs&, hipStream_t);

int max_nn_count(int elem_size, int R) {
  return largest_k([&](int k) { return (elem_size == 4 ? fused_lds_bytes<float>(k, R, 8) : fused_lds_bytes<double>(k, R, 8)) <= kCuLdsBytes; });
}
// the largest k at which the general-smoothness launch fits: the same with the node table
int max_nn_count_gen(int elem_size, int R) {
  return largest_k([&](int k) {
    return (elem_size == 4 ? fused_lds_bytes<float>(k, R, 8) : fused_lds_bytes<double>(k, R, 8)) + gen_table_bytes(elem_size) <= kCuLdsBytes;
  });
}

}  // namespace mgp
