// Backward (vector-Jacobian product) of one response's posterior mean / variance / y^T K^-1 y with respect to the
// HYPER-PARAMETERS -- length scale(s), the noise diagonal, the neighbours' responses -- for the fp64 static shapes of the
// dealt-triangle forward kernels (BASELINE config 4: anisotropic Matern, k = 50, d = 8: the gradient of the LOOCV
// objective that L-BFGS-B and the torch layer ask for; round 6), and, further down, for the row-per-lane static shapes
// of either element type (config 3: k = 30, d = 40) -- those with the FEATURE cotangents as well.
//
// Reference: torch autograd over src/MuyGPyS/torch/muygps_layer.py:129-164 (the reference's way to these gradients);
// the numpy chassis has only finite differences (src/MuyGPyS/_src/optimize/chassis/numpy.py:57-81).  The maths is
// mgp_backward.hip's:  a = K^-1 c, u = K^-1 y,  K-bar_ij = 2 gv a_i a_j - gm (a_i u_j + a_j u_i) - 2 gy u_i u_j,
// c-bar_j = gm u_j - 2 gv a_j,  q_ij = K-bar_ij dk/dacc_ij,  dL/dl_f = -(2 / l_f) sum_pairs q_ij (z_if - z_jf)^2.
//
// The kernel IS the forward kernel (mgp_fused_wave_kernel.h, BWD instantiation): gather, pair distances (kept in
// registers), covariances, the dealt lower triangle and its elimination -- 434 FMAs per neighbourhood instead of the
// 1 400 of a row per lane -- with every finished column written back into the dealt image, which so becomes the
// factor; then back-substitution for the two vectors on that image, the pair cotangents in the pair scheme's own
// layout, and the length-scale partials from the tile.  Two waves per SIMD; round 5's row-per-lane kernel
// (mgp_backward_wave.hip: a 64-double row, 32 kept distances, the multipliers in a 34 KB LDS matrix) ran at one:
// 117.7 ms per 2 M neighbourhoods against a 12.9 ms forward.
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "mgp_fused_wave_launch.h"

namespace mgp {

static void bwd_args(const BackwardArgs& b, FusedArgs* a) {
  *a = b.f;
  a->mean = a->var = a->ykinvy = nullptr;
  a->coeffs = nullptr;
  a->tree = LoocvTree{};
  a->packed_q = a->packed_nn = nullptr;
  a->bwd_gmean = b.grad_mean;
  a->bwd_gvar = b.grad_var;
  a->bwd_gyk = b.grad_yk;
  a->bwd_gls = b.grad_ls;
  a->bwd_gnz = b.grad_noise;
  a->bwd_gtg = b.grad_targets;
  a->bwd_gnn = b.grad_feat_nn;
  a->bwd_gq = b.grad_feat_q;
}

// one launch of a BWD instantiation, built in (`const void*`) or compiled at run time (hipFunction_t)
template <typename Kernel>
static int launch_bwd(Kernel fn, Residency& res, const BackwardArgs& b, const WaveShape& s, hipStream_t stream) {
  FusedArgs a;
  bwd_args(b, &a);
  WaveLaunch w = wave_geometry(a, s);
  if (w.status != MGP_OK) return w.status;
  return wave_launch(fn, res, a, s, w, stream);
}

// the shapes the library is built with (wave_builtin): fp64 k = 50, d = 8 on the dealt triangle (64 slots), fp32 k = 30,
// d = 40 row per lane (32 slots)
template <typename T, int NP, int KFIX, int DFIX, bool GRAM>
static int launch_bwd_builtin(const BackwardArgs& b, hipStream_t stream) {
  constexpr WaveShape S{(int)sizeof(T), NP, KFIX, 1, DFIX, true, false, false, GRAM, false, true, false};
  static_assert(wave_dims(S).STAT && wave_dims(S).DLT == (NP == 64), "the dealt-triangle shapes have 64 slots, the row-per-lane ones 32");
  static Residency res;
  return launch_bwd(reinterpret_cast<const void*>(&fused_wave_kernel<T, NP, KFIX, 1, DFIX, true, false, false, GRAM, false, true>), res, b, S,
                    stream);
}

// Static shapes the library was not built with: the BWD instantiation compiled at run time (mgp_jit.hip: one second per
// shape, cached on disk) -- as launch_jit of mgp_fused_wave.hip does for the forward kernels.
static bool dlt_shape(int k, int d) {  // fp64, one response: 33 .. 64 slots, rows of whole 16-byte groups, one feature stage
  return k + 2 >= 33 && k + 2 <= 64 && d >= 2 && d % 2 == 0 && (d + 3) / 4 * 4 <= 64;
}
// ---- row-per-lane form: 32-slot static shapes of either element type (BASELINE config 3's k = 30, d = 40 built in) ----
// slots of the row-per-lane instantiation that serves a shape (0: none): 32 for up to 32 rows (smaller neighbourhoods
// ride in the 32-slot kernel: lanes idle, nothing else changes), 64 for fp32 beyond; rows of whole 16-byte groups, one
// feature stage
static int row_slots(int es, int k, int d) {
  const int E = 16 / es, CH = 2 * E;
  const int DCAP = es == 4 ? 128 : 64;  // (fp32: rows of up to 128 features in one stage)
  if (k < 3 || d < E || d % E != 0 || (d + CH - 1) / CH * CH > DCAP) return 0;
  if (k + 2 <= 32) return 32;
  return (es == 4 && k + 2 <= 64) ? 64 : 0;
}
template <typename T>
static int launch_bwd_jit(const BackwardArgs& b, bool dlt, hipStream_t stream) {
  const FusedArgs& f = b.f;
  const int NP = dlt ? 64 : row_slots(sizeof(T), f.k, f.d);
  if (NP == 0 || jit_mode() == 0) return MGP_EUNSUPPORTED;
  const WaveShape s{(int)sizeof(T), NP, f.k, 1, f.d, true, false, false, wave_gram(sizeof(T), f.kernel_id, f.smoothness, true), false, true, true};
  if (wave_dims(s).DLT != dlt || !wave_dims(s).STAT) return MGP_EUNSUPPORTED;
  hipFunction_t fn = nullptr;
  const int jrc = jit_wave_function(s.es, NP, f.k, 1, f.d, false, s.gram, &fn, jit_mode() == 2 || f.b >= jit_min_batch(), false, true);
  if (jrc != MGP_OK) return jrc;
  static Residency res_dlt, res_row;  // (one per run-time compiled family)
  return launch_bwd(fn, dlt ? res_dlt : res_row, b, s, stream);
}

int prepare_backward_fwd(int elem_size, int k, int d, int kernel_id) {
  const bool dlt = elem_size == 8 && dlt_shape(k, d) && wave_dims(8, 64, k, 1, d, false, false).DLT;
  const int np = dlt ? 64 : ((elem_size == 4 || elem_size == 8) ? row_slots(elem_size, k, d) : 0);
  if (np == 0) return MGP_EUNSUPPORTED;
  const bool gram = wave_gram(elem_size, kernel_id, 1.0, true);
  if (wave_builtin(elem_size, k, 1, d, gram, false, true)) return MGP_OK;
  return jit_wave_prepare(elem_size, np, k, 1, d, false, gram, false, true);
}

// gradients of one response; plain tables, 16-byte aligned rows (feature cotangents: the row-per-lane shapes only)
template <typename T>
int launch_backward_fwd(const BackwardArgs& b, hipStream_t stream) {
  const FusedArgs& f = b.f;
  // (several responses: one combined right-hand side Y g_mean, formed as the rows' responses are fetched; the LOOCV form
  // with its y^T K^-1 y is one response by definition)
  if (f.R < 1 || (f.R != 1 && b.grad_yk) || f.targets_batch || f.kernel_id == MGP_KERNEL_MATERN_GEN) return MGP_EUNSUPPORTED;
  const bool feat = b.grad_feat_q != nullptr || b.grad_feat_nn != nullptr;  // feature cotangents: the row-per-lane form has them
  if (f.ls_count != 1 && f.ls_count != f.d) return MGP_EUNSUPPORTED;
  if (wave_align(f, false) % 16 != 0 || f.b >= ((int64_t)1 << 31)) return MGP_EUNSUPPORTED;
  static const bool off = getenv("MGP_BACKWARD_DLT") != nullptr && atoi(getenv("MGP_BACKWARD_DLT")) == 0;  // A/B switch (timing only)
  if (off) return MGP_EUNSUPPORTED;
  const bool builtin = wave_builtin(sizeof(T), f.k, 1, f.d, wave_gram(sizeof(T), f.kernel_id, f.smoothness, true), false, true);
  if constexpr (sizeof(T) == 8) {
    if (feat && row_slots(8, f.k, f.d) == 0) return MGP_EUNSUPPORTED;
    if (builtin) return launch_bwd_builtin<double, 64, 50, 8, false>(b, stream);
    if (dlt_shape(f.k, f.d)) return launch_bwd_jit<T>(b, true, stream);
  } else {
    if (builtin) return launch_bwd_builtin<float, 32, 30, 40, true>(b, stream);
  }
  return launch_bwd_jit<T>(b, false, stream);
}
template int launch_backward_fwd<float>(const BackwardArgs&, hipStream_t);
template int launch_backward_fwd<double>(const BackwardArgs&, hipStream_t);

}  // namespace mgp
