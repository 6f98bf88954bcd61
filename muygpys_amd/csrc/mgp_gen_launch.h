// General-smoothness Matern inside a fused kernel (matern_gen_eval / matern_gen_batch64, mgp_wave_common.h): the ONE
// host place that turns a smoothness into the launch constants the in-kernel evaluators read -- node spacing, the
// logarithm of h 2^(1-nu) / Gamma(nu) and, in fp64, the smallest scaled distance the node table covers -- and that knows
// what the node table costs in LDS.  Shared by the wave launcher (mgp_fused_wave_launch.h: the constants go into
// WaveGeom) and the launchers of the two workgroup families (mgp_generic.hip, mgp_large.hip: they go to the kernel as
// a GenLaunch argument of its own).
#pragma once
#include <cmath>

#include "mgp_assemble.h"
#include "mgp_wave_common.h"

namespace mgp {

// What a general-smoothness instantiation of a workgroup kernel is handed next to FusedArgs (the smoothness itself
// is FusedArgs::smoothness).  The closed-form instantiations receive a zeroed one and read nothing of it.
struct GenLaunch {
  double h64, lc64, xmin64;  // fp64: spacing, ln(h 2^(1-nu) / Gamma(nu)), smallest x of the table
  float h, lc;               // fp32: spacing, log2(h 2^(1-nu) / Gamma(nu))
  int tab;                   // byte offset of the node table in dynamic LDS (behind everything else)
  int dtab;                  // ... and of the derivative table behind it (the backward, mgp_backward_gen_large.hip)
  double psi;                // digamma(nu): dk/dnu (read by the backward alone)
};

// digamma(x), x > 0: the recurrence psi(x) = psi(x + 1) - 1 / x up to x >= 10, then the asymptotic series (its first
// omitted term is below 1e-13 there)
inline double gen_digamma(double x) {
  double s = 0.0;
  while (x < 10.0) {
    s -= 1.0 / x;
    x += 1.0;
  }
  const double f = 1.0 / (x * x);
  return s + log(x) - 0.5 / x - f * (1.0 / 12 - f * (1.0 / 120 - f * (1.0 / 252 - f * (1.0 / 240 - f * (1.0 / 132)))));
}

// the constants of one smoothness; fp64 = false leaves the fp64 members at values no kernel reads
inline GenLaunch gen_launch_constants(double nu, bool fp64) {
  GenLaunch g{0.3, 0.0, 1e-12, 0.5f, 0.0f, 0, 0, 0.0};
  const double h = gen_step(nu);
  g.psi = gen_digamma(nu);
  g.h = (float)h;
  g.lc = (float)((log(h) + (1.0 - nu) * log(2.0) - lgamma(nu)) / log(2.0));
  if (fp64) {  // finer step, natural logarithms, a larger table
    const double h64 = gen_step64(nu);
    g.h64 = h64;
    g.lc64 = log(h64) + (1.0 - nu) * log(2.0) - lgamma(nu);
    g.xmin64 = gen_xmin64(nu);
  }
  return g;
}

// bytes of the node table: 2 x MGP_GEN_NODES floats / 2 x MGP_GEN_NODES64 doubles
inline size_t gen_table_bytes(int elem_size) {
  return elem_size == 8 ? 2 * MGP_GEN_NODES64 * sizeof(double) : 2 * MGP_GEN_NODES * sizeof(float);
}

// pairs one thread hands the evaluator per call (NS of matern_gen_eval, CB of matern_gen_batch64) in the workgroup
// kernels.  The covariance strip of a workgroup is its thread count times this.
template <typename T>
constexpr int gen_pairs_per_call() { return sizeof(T) == 4 ? 4 : 2; }

// The covariance phase of a general-smoothness workgroup kernel: the (k+1) k / 2 squared distances of the strict lower
// triangle, found through at(row, col), become covariances in place.  The evaluators end their node loop on a wave
// ballot, so every thread of the workgroup makes the same number of calls: the pair index is strip-mined, a strip =
// NT threads x PC pairs, pair p0 + u NT + tid is thread tid's u-th; pairs past the end are dead in `live` (evaluated
// at x = 1, never stored).  The map is a function of k and NT alone, and a pair's value depends on the node count of
// its wave: a neighbourhood's bits do not depend on where in a batch, a grid or a workspace it is computed.
// Strip sizes: NT = 64 / 256 (mgp_generic.hip) or 256 / 512 (mgp_large.hip) times PC = 4 (fp32) / 2 (fp64).
template <typename T, typename At>
__device__ __forceinline__ void gen_covariance_phase(At at, int k, int metric_id, T post_scale, double nu, const GenLaunch& g,
                                                     const T* tab, int tid, int NT) {
  constexpr int PC = gen_pairs_per_call<T>();
  const int npairs = (k + 1) * k / 2;
  for (int p0 = 0; p0 < npairs; p0 += NT * PC) {  // (uniform trip count)
    T v[PC];
    T* dst[PC];
    unsigned live = 0;
#pragma unroll
    for (int u = 0; u < PC; ++u) {
      const int p = p0 + u * NT + tid;
      v[u] = T(1);
      dst[u] = nullptr;
      if (p < npairs) {
        int a_, c_;
        tri_decode(p, a_, c_);
        dst[u] = at(a_, c_);
        v[u] = *dst[u];
        live |= 1u << u;
      }
    }
    if constexpr (sizeof(T) == 4) {
#pragma unroll
      for (int u = 0; u < PC; ++u) v[u] = metric_arg<T>(v[u], metric_id, post_scale);
      matern_gen_eval<PC>(v, live, tab, (float)nu, g.h, g.lc);
    } else {
      if (metric_id == MGP_METRIC_L2) metric_batch64<PC, MGP_METRIC_L2>(v, post_scale);
      else metric_batch64<PC, MGP_METRIC_F2>(v, post_scale);
      matern_gen_batch64<PC>(v, live, tab, nu, g.h64, g.lc64, g.xmin64);
    }
#pragma unroll
    for (int u = 0; u < PC; ++u)
      if ((live >> u) & 1u) *dst[u] = v[u];
  }
}

// the node table of the launch's smoothness, once per workgroup (visible behind the next barrier)
template <typename T>
__device__ __forceinline__ void gen_build_node_table(T* tab, double nu, const GenLaunch& g, int tid) {
  if (tid >= MGP_WAVE) return;
  if constexpr (sizeof(T) == 4) gen_build_table(tab, (float)nu, g.h, tid);
  else gen_build_table64(tab, nu, g.h64, tid);
}

// bytes of the derivative table (gen_build_deriv_table / gen_build_deriv_table64): two more columns per node
inline size_t gen_deriv_table_bytes(int elem_size) { return gen_table_bytes(elem_size); }

// both tables of the backward, once per workgroup (visible behind the next barrier)
template <typename T>
__device__ __forceinline__ void gen_build_deriv_node_table(T* dtab, double nu, const GenLaunch& g, int tid) {
  if (tid >= MGP_WAVE) return;
  if constexpr (sizeof(T) == 4) gen_build_deriv_table(dtab, (float)nu, g.h, tid);
  else gen_build_deriv_table64(dtab, nu, g.h64, tid);
}

// The derivatives of one strip of pairs (gen_covariance_phase's strip: NT threads x PC pairs, pair p0 + u NT + tid is
// thread tid's u-th): v[u] = metric argument in, dk/dr out; dnu[u] = dk/dnu when NU.  Every thread of the workgroup
// calls this the same number of times.
template <typename T, bool NU>
__device__ __forceinline__ void gen_deriv_strip(T (&v)[gen_pairs_per_call<T>()], T (&dnu)[gen_pairs_per_call<T>()], unsigned live,
                                                double nu, const GenLaunch& g, const T* tab, const T* dtab) {
  constexpr int PC = gen_pairs_per_call<T>();
  if constexpr (sizeof(T) == 4) matern_gen_deriv_eval<PC, NU>(v, dnu, live, tab, dtab, (float)nu, g.h, g.lc, (float)g.psi);
  else matern_gen_deriv_batch64<PC, NU>(v, dnu, live, tab, dtab, nu, g.h64, g.lc64, g.xmin64, g.psi);
}

// the general-smoothness launches of the workgroup families (mgp_generic.hip, mgp_large.hip); a.smoothness is set
template <typename T> int launch_fused_generic_gen(const FusedArgs&, hipStream_t);
template <typename T> int launch_fused_large_gen(const FusedArgs&, void* workspace, int64_t workspace_bytes, hipStream_t);
int max_nn_count_gen(int elem_size, int R);
// ... and the per-neighbourhood-scale launches of the same two families (NsLaunch, mgp_assemble.h): closed-form kernels,
// ls_batch (b, a.ls_count) on the device; MGP_EUNSUPPORTED as the scalar launches of the same family
template <typename T> int launch_fused_generic_ns(const FusedArgs&, const void* ls_batch, hipStream_t);
template <typename T>
int launch_fused_large_ns(const FusedArgs&, const void* ls_batch, void* workspace, int64_t workspace_bytes, hipStream_t);
// ... and of the hyper-parameter backward on the slab factor (mgp_backward_gen_large.hip): grad_nu (b) may be NULL
template <typename T> int launch_hyper_backward_gen_large(const BackwardArgs&, void* grad_nu, void* workspace, int64_t workspace_bytes, hipStream_t);
int backward_gen_large_max_nn_count(int elem_size);
// ... and of the whole vector-Jacobian product in LDS (mgp_backward_gen.hip): two tables, every cotangent of
// BackwardArgs, grad_nu (b) may be NULL; MGP_EUNSUPPORTED beyond max_nn_count_backward_gen
template <typename T> int launch_backward_gen(const BackwardArgs&, void* grad_nu, hipStream_t);
int max_nn_count_backward_gen(int elem_size);
// ... and of the prediction from precomputed coefficients (mgp_fast_mean.hip): launch_fast_mean's arguments with the
// smoothness in place of the kernel id
template <typename T>
int launch_fast_mean_gen(const void* feat_q, const void* feat_nn, int d, const int64_t* batch_idx, const int64_t* nn_idx, int64_t b,
                         int k, const void* coeffs, const int64_t* coeff_row, int R, double smoothness, int metric_id,
                         const void* length_scale, int ls_count, void* mean, hipStream_t stream);

}  // namespace mgp
