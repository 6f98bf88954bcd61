// Generic (any nn_count that fits LDS) kernels of the local-GP hot path:
//   * fused gather -> distances -> kernel -> nugget -> factor -> mean/var/yKinvy
//   * the same factorisation on a materialised Kin (API parity: S1/S2/S3 + fast precompute)
// One workgroup owns one neighbourhood at a time; its whole local system lives in LDS
// (see mgp_lds_factor.h).  The specialised register-resident kernels in mgp_fused_wave.hip
// take over for the shapes they cover; this file is the path for everything else.
#include "mgp_args.h"
#include "mgp_gen_launch.h"
#include "mgp_launch.h"
#include "mgp_lds_factor.h"

namespace mgp {

// feature-tile row stride for a chunk of dc features (dc a multiple of 2E): 16-byte aligned rows, odd
// number of 16-byte slots
template <typename T>
__host__ __device__ inline int tile_row_stride(int dc) { return dc + 16 / (int)sizeof(T); }

// dynamic LDS carve (every array 16-byte aligned):
// [idx: (k+2 & ~1) int64][S: rows*SP T][X: (k+1)*XP T][il: dc T][piv: k T][flag]
// GEN (the general-smoothness Matern, a.smoothness): + [node table: 2 MGP_GEN_NODES float / 2 MGP_GEN_NODES64 double]
// at byte g.tab, behind everything else; the closed-form instantiations reserve and read nothing of `g`.
template <typename T, bool GEN>
__device__ __forceinline__ void fused_generic_body(const FusedArgs& a, const GenLaunch& g) {
  using V = typename lds_vec<T>::type;
  constexpr int E = 16 / (int)sizeof(T);
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int k = a.k, d = a.d, R = a.R, dc = a.dc;
  const int rows = k + 1 + R;
  const int SP = lds_row_stride<T>(k);
  const int XP = tile_row_stride<T>(dc);
  int64_t* idx = reinterpret_cast<int64_t*>(smem);
  T* S = reinterpret_cast<T*>(idx + ((k + 2) & ~1));
  T* X = S + rows * SP;
  T* il = X + (k + 1) * XP;
  T* piv = il + dc;
  int* flag = reinterpret_cast<int*>(piv + k);

  const T* feat_q = static_cast<const T*>(a.feat_q);
  const T* feat_nn = static_cast<const T*>(a.feat_nn);
  const T* targets = static_cast<const T*>(a.targets);
  const T* noise_dev = static_cast<const T*>(a.noise_dev);
  const T* ls = static_cast<const T*>(a.length_scale);
  const int tid = threadIdx.x, NT = blockDim.x;
  const bool aniso = a.ls_count > 1;
  const int npairs = (k + 1) * k / 2;
  const bool vec_ok = d % E == 0 && dc % E == 0 && ((uintptr_t)feat_q | (uintptr_t)feat_nn) % 16 == 0;

  T post_scale = T(1);
  if (!aniso) {
    const T l = ls[0];
    post_scale = a.metric_id == MGP_METRIC_L2 ? T(1) / l : T(1) / (l * l);
  }
  if constexpr (GEN) gen_build_node_table<T>(reinterpret_cast<T*>(smem + g.tab), a.smoothness, g, tid);

  for (int64_t nb = blockIdx.x; nb < a.b; nb += gridDim.x) {
    __syncthreads();  // previous neighbourhood fully consumed
    for (int r = tid; r <= k; r += NT)
      idx[r] = r < k ? a.nn_idx[nb * k + r] : (a.batch_idx ? a.batch_idx[nb] : nb);
    __syncthreads();

    for (int d0 = 0; d0 < d; d0 += dc) {
      const int w = min(dc, d - d0);
      const int wp = (w + E - 1) / E * E;  // zero-padded to whole 16-byte pieces
      // coalesced gather of the (k+1) x w feature tile: consecutive lanes walk a row
      gather_tile_lds<T>(X, XP, feat_q, feat_nn, idx, k, d, d0, w, wp, vec_ok, tid, NT);
      if (aniso)
        for (int c = tid; c < wp; c += NT) il[c] = c < w ? T(1) / ls[d0 + c] : T(0);
      __syncthreads();
      for (int p = tid; p < npairs; p += NT) {
        // p -> (row a_, col c_) of the strict lower triangle of the (k+1)-point set
        int a_ = (int)((1.0f + sqrtf(1.0f + 8.0f * (float)p)) * 0.5f);
        while (a_ * (a_ - 1) / 2 > p) --a_;
        while ((a_ + 1) * a_ / 2 <= p) ++a_;
        const int c_ = p - a_ * (a_ - 1) / 2;
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
        T* dst = S + a_ * SP + c_;
        *dst = d0 == 0 ? acc : *dst + acc;
      }
      __syncthreads();
    }
    // distances -> covariances (in place), nugget on the diagonal, responses into the tail rows
    if constexpr (GEN) {
      // (whole strips of NT x 4 / NT x 2 pairs, every thread in every evaluator call: mgp_gen_launch.h)
      gen_covariance_phase<T>([&](int r, int c) { return S + r * SP + c; }, k, a.metric_id, post_scale, a.smoothness, g,
                              reinterpret_cast<const T*>(smem + g.tab), tid, NT);
    } else {
      for (int p = tid; p < npairs; p += NT) {
        int a_ = (int)((1.0f + sqrtf(1.0f + 8.0f * (float)p)) * 0.5f);
        while (a_ * (a_ - 1) / 2 > p) --a_;
        while ((a_ + 1) * a_ / 2 <= p) ++a_;
        const int c_ = p - a_ * (a_ - 1) / 2;
        T* dst = S + a_ * SP + c_;
        *dst = kernel_eval<T>(a.kernel_id, metric_arg<T>(*dst, a.metric_id, post_scale));
      }
    }
    for (int r = tid; r < k; r += NT) {
      T eps;
      if (a.noise_mode == MGP_NOISE_SCALAR) eps = (T)a.noise_scalar;
      else if (a.noise_mode == MGP_NOISE_TABLE) eps = noise_dev[idx[r]];
      else eps = noise_dev[nb * k + r];
      S[r * SP + r] = T(1) + eps;  // kernel(0) == 1 for every kernel on the path
    }
    for (int t = tid; t < k * R; t += NT) {
      const int c = t / R, r = t - c * R;
      S[(k + 1 + r) * SP + c] = targets[(a.targets_batch ? nb * k + c : idx[c]) * (int64_t)R + r];
    }
    __syncthreads();
    const bool bad = factor_augmented_lds<T>(S, SP, k, rows, piv, flag, tid, NT);
    T* mean = static_cast<T*>(a.mean);
    T* var = static_cast<T*>(a.var);
    T* yk = static_cast<T*>(a.ykinvy);
    emit_outputs_lds<T>(S, SP, k, R, T(1), bad, true, mean ? mean + nb * R : nullptr, var ? var + nb : nullptr,
                        yk ? yk + nb * R : nullptr, tid, NT);
    if (bad && tid == 0 && a.info) atomicAdd(a.info, 1);
  }
}

// the closed-form kernels, and the general-smoothness Matern under a name of its own (its constants: an argument of
// its own)
template <typename T>
__global__ void fused_generic_kernel(FusedArgs a) { fused_generic_body<T, false>(a, GenLaunch{}); }
template <typename T>
__global__ void fused_generic_gen_kernel(FusedArgs a, GenLaunch g) { fused_generic_body<T, true>(a, g); }

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
    emit_outputs_lds<T>(S, SP, k, R, (T)a.kout, bad, Kcross != nullptr, mean ? mean + nb * R : nullptr,
                        var ? var + nb : nullptr, yk ? yk + nb * R : nullptr, tid, NT);
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
  const LaunchLabel label(a.b, a.k, a.d, a.R, "mgp::fused_generic%s_kernel<%s>", GEN ? "_gen" : "", sizeof(T) == 4 ? "float" : "double");
  const int threads = lds_factor_threads(a.k + 1 + a.R);
  if constexpr (GEN) return launch_capacity(&fused_generic_gen_kernel<T>, threads, fc.lds, a.b, Capacity{16}, stream, &label, a, g).status;
  else return launch_capacity(&fused_generic_kernel<T>, threads, fc.lds, a.b, Capacity{16}, stream, &label, a).status;
}
template <typename T>
int launch_fused_generic(const FusedArgs& a, hipStream_t stream) { return launch_fused_generic_impl<T, false>(a, stream); }
template <typename T>
int launch_fused_generic_gen(const FusedArgs& a, hipStream_t stream) { return launch_fused_generic_impl<T, true>(a, stream); }

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
