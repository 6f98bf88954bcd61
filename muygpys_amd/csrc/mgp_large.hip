// Local systems beyond LDS (k + 1 + R <= kLargeMaxRows = 1024): the work of mgp_generic.hip -- gather -> distances ->
// kernel -> nugget -> augmented factorisation -> mean / var / yKinvy, and the same factorisation on a materialised
// Kin -- with the system in GLOBAL memory: one slab of a caller-provided workspace per workgroup of the persistent
// grid.  No workgroup waits on another; what a neighbourhood returns depends on nothing but its own inputs.
//
// Slab: the lower trapezoid of the augmented system of mgp_lds_factor.h, row by row.  Row i < k holds its columns up
// to the end of its 32-column block (32 (i / 32 + 1) elements), the 1 + R trailing rows hold KP = 32 ceil(k / 32)
// each; every row starts on a 128-byte boundary.  What lies right of the diagonal inside a diagonal block is never
// initialised and never reaches a result (see factor_augmented_slab).
//
// Factorisation: left-looking by panels of LNB = 32 columns.  Per panel (first column j0):
//   1. update   S[i][j0 + n] -= sum_{c < j0} S[i][c] S[j0 + n][c]  for every row i >= j0, the trailing rows included
//               (the forward substitution of z and the responses "for free") -- a tiled GEMM on the matrix pipe,
//               one tile of rows per wave, accumulators in registers over the whole c loop, operands streamed from
//               the slab (L2): v_mfma_f32_32x32x2_f32 (bit for bit an fmaf chain) / v_mfma_f64_16x16x4_f64.
//               This is the k^3 / 3 of the factorisation.
//   2. the 32 x 32 diagonal block is factorised by EVERY wave, redundantly, in registers (lane = row, the column
//      broadcasts are v_readlane: no LDS round trip and no barrier inside the block), as factor_augmented_rows does
//      with its 4 x 4 block; the first wave's copy goes back to the slab and into LDS
//   3. every row below the block forward-substitutes its 32 panel entries, one row per thread, the block's rows
//      coming out of LDS as 16-byte broadcasts
// Four workgroup barriers per panel.  The diagonal holds the INVERSE pivots afterwards (nothing reads the diagonal of
// L but the back-substitution of the coefficient output, which wants the inverse).
#include "mgp_assemble.h"
#include "mgp_gen_launch.h"
#include "mgp_large_factor.h"

namespace mgp {

// The general-smoothness instantiations keep the body they had before the closed-form kernels' front end moved to
// mgp_assemble.h (its chunk loop, nugget and responses written out): on the shared one fused_large_gen_kernel<float>
// measured 0.3 - 0.4 % behind this code at k = 300, d = 8, outside its own run-to-run spread, though the loops that take
// the time were the same instructions.  A model parameter that touches the assembly is written here as well.
// (LDS carve: as fused_large_body below, + the node table at byte g.tab, behind everything else)
// COEFFS: as in fused_large_body (mgp_fast_coefficients_gen_*), an instantiation of its own.
template <typename T, bool COEFFS = false>
__device__ __forceinline__ void fused_large_gen_body(const FusedArgs& a, T* workspace, int slab_elems, const GenLaunch& g) {
  using V = typename lds_vec<T>::type;
  constexpr int E = 16 / (int)sizeof(T);
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int k_ = a.k, d = a.d, R_ = a.R, dc = a.dc;
  const int XP = dc + E;  // feature-tile row stride: 16-byte aligned rows, odd number of 16-byte slots (dc % (2 E) == 0)
  T* Lb = reinterpret_cast<T*>(smem);
  int64_t* idx = reinterpret_cast<int64_t*>(Lb + LNB * large_lp<T>());
  T* X = reinterpret_cast<T*>(idx + ((k_ + 2) & ~1));
  T* il = X + (k_ + 1) * XP;

  const T* feat_q = static_cast<const T*>(a.feat_q);
  const T* feat_nn = static_cast<const T*>(a.feat_nn);
  const T* targets = static_cast<const T*>(a.targets);
  const T* noise_dev = static_cast<const T*>(a.noise_dev);
  const T* ls = static_cast<const T*>(a.length_scale);
  const int tid = threadIdx.x, NT = blockDim.x;
  const bool aniso = a.ls_count > 1;
  const bool vec_ok = d % E == 0 && dc % E == 0 && ((uintptr_t)feat_q | (uintptr_t)feat_nn) % 16 == 0;

  T post_scale = T(1);
  if (!aniso) {
    const T l = ls[0];
    post_scale = a.metric_id == MGP_METRIC_L2 ? T(1) / l : T(1) / (l * l);
  }
  gen_build_node_table<T>(reinterpret_cast<T*>(smem + g.tab), a.smoothness, g, tid);

  for (int64_t nb = blockIdx.x; nb < a.b; nb += gridDim.x) {
    __syncthreads();  // previous neighbourhood fully consumed
    int k = k_, R = R_;
    asm volatile("" : "+s"(k), "+s"(R));
    const int rows = k + 1 + R;
    const int npairs = (k + 1) * k / 2;
    const SlabRows<T> row{workspace + (int64_t)blockIdx.x * slab_elems, k};
    if constexpr (COEFFS) fill_index_list_no_query(idx, a, nb, k, tid, NT);
    else fill_index_list(idx, a, nb, k, tid, NT);
    __syncthreads();
    // squared distances, one chunk of dc features at a time, the partial sums in the slab (pair_distances, written out)
    for (int d0 = 0; d0 < d; d0 += dc) {
      const int w = min(dc, d - d0);
      const int wp = (w + E - 1) / E * E;  // zero-padded to whole 16-byte pieces
      gather_tile_lds<T>(X, XP, feat_q, feat_nn, idx, k, d, d0, w, wp, vec_ok, tid, NT);
      if (aniso)
        for (int c = tid; c < wp; c += NT) il[c] = c < w ? T(1) / ls[d0 + c] : T(0);
      __syncthreads();
      for (int p = tid; p < npairs; p += NT) {
        int a_, c_;
        tri_decode(p, a_, c_);
        const T* xa = X + a_ * XP;
        const T* xc = X + c_ * XP;
        T acc = T(0);
        if (aniso) {
#pragma unroll 2
          for (int j = 0; j < wp; j += E) {
            const V df = (*reinterpret_cast<const V*>(xa + j) - *reinterpret_cast<const V*>(xc + j)) *
                         *reinterpret_cast<const V*>(il + j);
            acc += vec_dot(df, df);
          }
        } else {
#pragma unroll 2
          for (int j = 0; j < wp; j += E) {
            const V df = *reinterpret_cast<const V*>(xa + j) - *reinterpret_cast<const V*>(xc + j);
            acc += vec_dot(df, df);
          }
        }
        T* dst = row(a_) + c_;
        if (d0 > 0) acc += *dst;
        *dst = acc;  // (the covariances: a phase of its own below)
      }
      __syncthreads();
    }
    // distances out of the slab, covariances back into it, each pair by the thread that wrote its distance (whole
    // strips of NT x 4 / NT x 2 pairs, every thread in every evaluator call: mgp_gen_launch.h)
    gen_covariance_phase<T>([&](int r, int c) { return row(r) + c; }, k, a.metric_id, post_scale, a.smoothness, g,
                            reinterpret_cast<const T*>(smem + g.tab), tid, NT);
    for (int r = tid; r < k; r += NT) {
      T eps;
      if (a.noise_mode == MGP_NOISE_SCALAR) eps = (T)a.noise_scalar;
      else if (a.noise_mode == MGP_NOISE_TABLE) eps = noise_dev[idx[r]];
      else eps = noise_dev[nb * k + r];
      row(r)[r] = T(1) + eps;  // kernel(0) == 1 for every kernel on the path
    }
    for (int t = tid; t < k * R; t += NT) {
      const int c = t / R, r = t - c * R;
      row(k + 1 + r)[c] = targets[(a.targets_batch ? nb * k + c : idx[c]) * (int64_t)R + r];
    }
    __syncthreads();
    const bool bad = factor_augmented_slab<T>(row, k, rows, Lb, tid, NT);
    T* mean = static_cast<T*>(a.mean);
    T* var = static_cast<T*>(a.var);
    T* yk = static_cast<T*>(a.ykinvy);
    emit_outputs<T>(row, k, R, T(1), bad, true, mean ? mean + nb * R : nullptr, var ? var + nb : nullptr,
                    yk ? yk + nb * R : nullptr, tid);
    if constexpr (COEFFS) {
      if (a.coeffs)  // (the diagonal holds the inverse pivots)
        back_substitute_columns<T>(row, k, R, [&](int j) { return row(j)[j]; }, bad, static_cast<T*>(a.coeffs) + nb * (int64_t)k * R, tid, NT);
    }
    if (bad && tid == 0 && a.info) atomicAdd(a.info, 1);
  }
}

// dynamic LDS carve (every array 16-byte aligned): [Lb: LNB*LP T][idx: (k+2 & ~1) int64][X: (k+1)*XP T][il: dc T]
// COEFFS (a.coeffs set, no query, no mean / var / yKinvy: the fast-mean precompute): the back-substitution behind the
// factorisation, K^-1 y_r into a.coeffs (b, k, R) -- an instantiation of its own, as in mgp_generic.hip.
// NS (per-neighbourhood length scales, `n`: mgp_assemble.h): as in mgp_generic.hip, an instantiation of its own.
template <typename T, bool COEFFS = false, bool NS = false>
__device__ __forceinline__ void fused_large_body(const FusedArgs& a, T* workspace, int slab_elems, const NsLaunch& n = NsLaunch{}) {
  static_assert(!NS || !COEFFS, "per-neighbourhood scales: the posterior alone");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int k_ = a.k, R_ = a.R, dc = a.dc;
  const int XP = tile_row_stride<T>(dc);
  T* Lb = reinterpret_cast<T*>(smem);
  int64_t* idx = reinterpret_cast<int64_t*>(Lb + LNB * large_lp<T>());
  T* X = reinterpret_cast<T*>(idx + ((k_ + 2) & ~1));
  T* il = X + (k_ + 1) * XP;

  const int tid = threadIdx.x, NT = blockDim.x;
  T post_scale = T(1);
  if constexpr (!NS) post_scale = iso_scale<T, false>(a).post_scale;
  const T* ls = static_cast<const T*>(a.length_scale);  // (NS: row nb of n.ls_batch, per neighbourhood)

  for (int64_t nb = blockIdx.x; nb < a.b; nb += gridDim.x) {
    __syncthreads();  // previous neighbourhood fully consumed
    int k = k_, R = R_;
    asm volatile("" : "+s"(k), "+s"(R));
    const int rows = k + 1 + R;
    const SlabRows<T> row{workspace + (int64_t)blockIdx.x * slab_elems, k};
    if constexpr (COEFFS) fill_index_list_no_query(idx, a, nb, k, tid, NT);
    else fill_index_list(idx, a, nb, k, tid, NT);
    __syncthreads();
    if constexpr (NS) {
      // a scale that is not finite and > 0: NaN outputs and one count in info, like a non-positive pivot
      bool bad_scale;
      ls = ns_select_scales<T>(a, n, nb, &bad_scale);
      if (bad_scale) {
        ns_refuse_neighbourhood<T>(a, nb, R, tid, NT);
        continue;
      }
      post_scale = iso_scale_at<T, false>(a, ls).post_scale;
    }

    // ---- assemble: the chunks' rows are staged in LDS, the partial sums of the squared distances live in the slab,
    // and the last chunk turns a distance into the covariance ----
    pair_distances_at<T>(a, ls, k, idx, X, XP, il, tid, NT, [&](int, int r, int c, T acc, int d0, bool last) {
      T* dst = row(r) + c;
      if (d0 > 0) acc += *dst;
      *dst = last ? kernel_eval<T>(a.kernel_id, metric_arg<T>(acc, a.metric_id, post_scale)) : acc;
    });
    fill_diagonal<T>(row, a, idx, nb, k, tid, NT);
    fill_responses<T>(row, a, idx, nb, k, R, tid, NT);
    __syncthreads();

    // ---- factor, finish ----
    const bool bad = factor_augmented_slab<T>(row, k, rows, Lb, tid, NT);
    T* mean = static_cast<T*>(a.mean);
    T* var = static_cast<T*>(a.var);
    T* yk = static_cast<T*>(a.ykinvy);
    emit_outputs<T>(row, k, R, T(1), bad, true, mean ? mean + nb * R : nullptr, var ? var + nb : nullptr,
                    yk ? yk + nb * R : nullptr, tid);
    if constexpr (COEFFS) {
      if (a.coeffs)  // (the diagonal holds the inverse pivots)
        back_substitute_columns<T>(row, k, R, [&](int j) { return row(j)[j]; }, bad, static_cast<T*>(a.coeffs) + nb * (int64_t)k * R, tid, NT);
    }
    if (bad && tid == 0 && a.info) atomicAdd(a.info, 1);
  }
}

// the closed-form kernels, the same with the coefficient output, and the general-smoothness Matern under a name of its
// own (its constants: an argument of its own)
template <typename T>
__global__ void __launch_bounds__(512) fused_large_kernel(FusedArgs a, T* workspace, int slab_elems) {
  fused_large_body<T>(a, workspace, slab_elems);
}
template <typename T>
__global__ void __launch_bounds__(512) fused_large_coeffs_kernel(FusedArgs a, T* workspace, int slab_elems) {
  fused_large_body<T, true>(a, workspace, slab_elems);
}
template <typename T>
__global__ void __launch_bounds__(512) fused_large_ns_kernel(FusedArgs a, T* workspace, int slab_elems, NsLaunch n) {
  fused_large_body<T, false, true>(a, workspace, slab_elems, n);
}
template <typename T>
__global__ void __launch_bounds__(512) fused_large_gen_kernel(FusedArgs a, T* workspace, int slab_elems, GenLaunch g) {
  fused_large_gen_body<T>(a, workspace, slab_elems, g);
}
template <typename T>
__global__ void __launch_bounds__(512) fused_large_gen_coeffs_kernel(FusedArgs a, T* workspace, int slab_elems, GenLaunch g) {
  fused_large_gen_body<T, true>(a, workspace, slab_elems, g);
}

template <typename T>
__global__ void __launch_bounds__(512) solve_large_kernel(SolveArgs a, T* workspace, int slab_elems) {
  const int k_ = a.k, R_ = a.R;
  const T* Kin = static_cast<const T*>(a.Kin);
  const T* Kcross = static_cast<const T*>(a.Kcross);
  const T* Y = static_cast<const T*>(a.Y);
  const int tid = threadIdx.x, NT = blockDim.x;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  T* Lb = reinterpret_cast<T*>(smem);  // the LDS copy of the diagonal block: all the LDS this front end needs

  for (int64_t nb = blockIdx.x; nb < a.b; nb += gridDim.x) {
    __syncthreads();
    int k = k_, R = R_;
    asm volatile("" : "+s"(k), "+s"(R));
    const int rows = k + 1 + R;
    const SlabRows<T> row{workspace + (int64_t)blockIdx.x * slab_elems, k};
    const T* Kb = Kin + nb * (int64_t)k * k;
    for (int t = tid; t < k * k; t += NT) {
      const int i = t / k, j = t - i * k;
      if (j <= i) row(i)[j] = Kb[t];  // lower triangle, as LAPACK 'L' would read it
    }
    for (int c = tid; c < k; c += NT) row(k)[c] = Kcross ? Kcross[nb * k + c] : T(0);
    for (int t = tid; t < k * R; t += NT) {
      const int c = t / R, r = t - c * R;
      row(k + 1 + r)[c] = Y[(nb * k + c) * (int64_t)R + r];
    }
    __syncthreads();
    const bool bad = factor_augmented_slab<T>(row, k, rows, Lb, tid, NT);
    T* mean = static_cast<T*>(a.mean);
    T* var = static_cast<T*>(a.var);
    T* yk = static_cast<T*>(a.ykinvy);
    emit_outputs<T>(row, k, R, (T)a.kout, bad, Kcross != nullptr, mean ? mean + nb * R : nullptr,
                    var ? var + nb : nullptr, yk ? yk + nb * R : nullptr, tid);
    if (a.coeffs) {
      // back-substitution of all R responses at once, in place in rows k+1+r (the diagonal holds the inverse pivots)
      back_substitute_columns<T>(row, k, R, [&](int j) { return row(j)[j]; }, bad, static_cast<T*>(a.coeffs) + nb * (int64_t)k * R, tid, NT);
    }
    if (bad && tid == 0 && a.info) atomicAdd(a.info, 1);
  }
}

// (kMaxWorkspace, kMaxPerCu, slab_count and slab_block_threads: mgp_large_factor.h, shared with the backward; the LDS of
// a CU, the feature chunk and the grid -- one workgroup per slab of the workspace, at most the resident capacity, at most
// b: mgp_launch.h)

template <typename T>
static size_t fused_lds_bytes(int k, int dc) {
  size_t n = (size_t)((k + 2) & ~1) * sizeof(int64_t);
  n += ((size_t)LNB * large_lp<T>() + (size_t)(k + 1) * tile_row_stride<T>(dc) + dc) * sizeof(T);
  return (n + 15) & ~(size_t)15;
}

int64_t large_slab_bytes(int elem_size, int k, int R) {
  // large_slab_elems in 64 bits (the C entries size-check a workspace before they refuse a k beyond the limit);
  // whole 256-byte lines: the slabs of neighbouring workgroups share none
  const int64_t q = k / LNB, r = k % LNB, kp = (q + (r ? 1 : 0)) * LNB;
  const int64_t elems = LNB * LNB * (q * (q + 1) / 2) + r * LNB * (q + 1) + (1 + (int64_t)R) * kp;
  if (elems > (INT64_MAX - 255) / elem_size) return INT64_MAX;  // (k or R near INT_MAX: no workspace holds a slab)
  return (elems * elem_size + 255) / 256 * 256;
}

int64_t large_workspace_bytes(int elem_size, int k, int R, int64_t b) {
  const int64_t slab = large_slab_bytes(elem_size, k, R), n = slab_count(b);
  return n * slab > kMaxWorkspace ? kMaxWorkspace : n * slab;
}

// GEN: the general-smoothness Matern (a.smoothness), which the closed-form entry refuses (it has no smoothness argument);
// its node table lies behind what the closed-form launch of the same shape and chunk takes
template <typename T, bool GEN>
static int launch_fused_large_impl(const FusedArgs& in, void* workspace, int64_t workspace_bytes, hipStream_t stream) {
  FusedArgs a = in;
  const int64_t rows = (int64_t)a.k + 1 + a.R;  // (64 bits: k or R near INT_MAX must not wrap past the limit)
  if (rows > kLargeMaxRows || (a.kernel_id == MGP_KERNEL_MATERN_GEN) != GEN) return MGP_EUNSUPPORTED;
  const int64_t slab = large_slab_bytes(sizeof(T), a.k, a.R);
  const size_t table = GEN ? gen_table_bytes(sizeof(T)) : 0;
  // feature chunk: a multiple of 8, as wide as fits the CU's LDS (one workgroup per CU: nothing to share it with; every
  // further chunk is one more pass over the slab's triangle: at k = 1000, d = 40 five chunks of 8 cost as much as
  // the factorisation), at least 8
  const FeatureChunk fc = feature_chunk(a.d, [&](int dc) { return fused_lds_bytes<T>(a.k, dc) + table; });
  if (!fc.fits) return MGP_EUNSUPPORTED;
  a.dc = fc.dc;
  GenLaunch g{};
  if (GEN) {
    g = gen_launch_constants(a.smoothness, sizeof(T) == 8);
    g.tab = (int)(fc.lds - table);
  }
  const LaunchLabel label(a.b, a.k, a.d, a.R, "mgp::fused_large%s%s_kernel<%s>", GEN ? "_gen" : "", a.coeffs ? "_coeffs" : "", sizeof(T) == 4 ? "float" : "double");
  const int threads = slab_block_threads((int)rows), slab_elems = (int)(slab / (int64_t)sizeof(T));
  const Capacity cap{kMaxPerCu, workspace_bytes / slab};
  if constexpr (GEN) {
    if (a.coeffs) return launch_capacity(&fused_large_gen_coeffs_kernel<T>, threads, fc.lds, a.b, cap, stream, &label, a, static_cast<T*>(workspace), slab_elems, g).status;
    return launch_capacity(&fused_large_gen_kernel<T>, threads, fc.lds, a.b, cap, stream, &label, a, static_cast<T*>(workspace), slab_elems, g).status;
  } else if (a.coeffs)
    return launch_capacity(&fused_large_coeffs_kernel<T>, threads, fc.lds, a.b, cap, stream, &label, a, static_cast<T*>(workspace), slab_elems).status;
  else
    return launch_capacity(&fused_large_kernel<T>, threads, fc.lds, a.b, cap, stream, &label, a, static_cast<T*>(workspace), slab_elems).status;
}
template <typename T>
int launch_fused_large(const FusedArgs& a, void* workspace, int64_t workspace_bytes, hipStream_t stream) {
  return launch_fused_large_impl<T, false>(a, workspace, workspace_bytes, stream);
}
template <typename T>
int launch_fused_large_gen(const FusedArgs& a, void* workspace, int64_t workspace_bytes, hipStream_t stream) {
  return launch_fused_large_impl<T, true>(a, workspace, workspace_bytes, stream);
}

// per-neighbourhood length scales: the slab, the LDS carve, the threads and the grid of the scalar launch
template <typename T>
int launch_fused_large_ns(const FusedArgs& in, const void* ls_batch, void* workspace, int64_t workspace_bytes, hipStream_t stream) {
  FusedArgs a = in;
  const int64_t rows = (int64_t)a.k + 1 + a.R;
  if (rows > kLargeMaxRows || a.kernel_id == MGP_KERNEL_MATERN_GEN || a.coeffs) return MGP_EUNSUPPORTED;
  const int64_t slab = large_slab_bytes(sizeof(T), a.k, a.R);
  const FeatureChunk fc = feature_chunk(a.d, [&](int dc) { return fused_lds_bytes<T>(a.k, dc); });
  if (!fc.fits) return MGP_EUNSUPPORTED;
  a.dc = fc.dc;
  a.length_scale = nullptr;  // (not read: the scales are the last argument's)
  const LaunchLabel label(a.b, a.k, a.d, a.R, "mgp::fused_large_ns_kernel<%s>", sizeof(T) == 4 ? "float" : "double");
  return launch_capacity(&fused_large_ns_kernel<T>, slab_block_threads((int)rows), fc.lds, a.b, Capacity{kMaxPerCu, workspace_bytes / slab},
                         stream, &label, a, static_cast<T*>(workspace), (int)(slab / (int64_t)sizeof(T)), NsLaunch{ls_batch}).status;
}

template <typename T>
int launch_solve_large(const SolveArgs& a, void* workspace, int64_t workspace_bytes, hipStream_t stream) {
  const int64_t rows = (int64_t)a.k + 1 + a.R;
  if (rows > kLargeMaxRows) return MGP_EUNSUPPORTED;
  const int64_t slab = large_slab_bytes(sizeof(T), a.k, a.R);
  const size_t lds = (size_t)LNB * large_lp<T>() * sizeof(T);
  return launch_capacity(&solve_large_kernel<T>, slab_block_threads((int)rows), lds, a.b, Capacity{kMaxPerCu, workspace_bytes / slab}, stream,
                         nullptr, a, static_cast<T*>(workspace), (int)(slab / (int64_t)sizeof(T))).status;
}

template int launch_fused_large<float>(const FusedArgs&, void*, int64_t, hipStream_t);
template int launch_fused_large<double>(const FusedArgs&, void*, int64_t, hipStream_t);
template int launch_fused_large_gen<float>(const FusedArgs&, void*, int64_t, hipStream_t);
template int launch_fused_large_gen<double>(const FusedArgs&, void*, int64_t, hipStream_t);
template int launch_fused_large_ns<float>(const FusedArgs&, const void*, void*, int64_t, hipStream_t);
template int launch_fused_large_ns<double>(const FusedArgs&, const void*, void*, int64_t, hipStream_t);
template int launch_solve_large<float>(const SolveArgs&, void*, int64_t, hipStream_t);
template int launch_solve_large<double>(const SolveArgs&, void*, int64_t, hipStream_t);

}  // namespace mgp
