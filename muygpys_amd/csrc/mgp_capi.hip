// extern "C" boundary: argument validation + dispatch to the kernels.  See
// include/muygpys_hip.h for the contract and the reference functions each entry replaces.
#include <cstdlib>
#include <cstdio>

#include "mgp_args.h"
#include "mgp_gen_launch.h"

#include <cstdarg>
#include <cstring>

namespace mgp {

static thread_local char g_last_kernel[256] = "";
static thread_local int g_tree_grid = 0, g_tree_nh = 0;
// how the one-launch LOOCV evaluation hands sums between workgroups (mgp_loocv_tree.h); process-wide
static int tree_mode_from_env() {
  const char* e = getenv("MUYGPYS_HIP_LOOCV_TREE");
  if (!e || !*e || !strcmp(e, "tickets")) return kTreeTickets;
  if (!strcmp(e, "fenced")) return kTreeFenced;
  if (!strcmp(e, "three_launch")) return kTreeThreeLaunch;
  fprintf(stderr, "mgp: MUYGPYS_HIP_LOOCV_TREE=%s is none of tickets / fenced / three_launch; using three_launch\n", e);
  return kTreeThreeLaunch;  // (an unknown word must not select the least conservative form)
}
static int g_tree_mode = tree_mode_from_env();
void note_tree_geometry(int grid, int nh) { g_tree_grid = grid, g_tree_nh = nh; }
static thread_local int64_t g_launch_grid = 0;
static thread_local int g_launch_lds = 0;
void note_launch_geometry(int64_t grid, size_t lds_bytes) { g_launch_grid = grid, g_launch_lds = (int)lds_bytes; }
void note_launch(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_last_kernel, sizeof(g_last_kernel), fmt, ap);
  va_end(ap);
}

static bool valid_kernel(int id) { return id >= MGP_KERNEL_RBF && id <= MGP_KERNEL_MATERN_INF; }
static bool valid_metric(int id) { return id == MGP_METRIC_L2 || id == MGP_METRIC_F2; }

#ifdef MGP_DEBUG_HOOKS
extern int g_phase_mask;  // mgp_fused_wave.hip (timing ablations, debug builds only)
extern int g_grid_per_cu;
extern int g_lds_pad;
extern int g_bwd_stage;  // mgp_backward.hip
#endif

// which kernel family serves a fused call: the dispatcher's choice, or one family named by the
// caller (mgp_posterior_generic_* / mgp_posterior_rhs_*: tests and A/B timing)
enum { PATH_AUTO = 0, PATH_GENERIC = 1, PATH_RHS = 2 };

// ---- the one path from the C arguments of a fused entry to FusedArgs -------------------------------------------------
// What an entry asks of the arguments the fused entries share.  Prepared tables need no flag (an entry that does not
// take them passes none), and neither does the response count: every entry needs R >= 1 (mgp_fast_coefficients_*
// passes its own 1).  A new model parameter is validated and assigned in fused_args, once.
enum {
  NEED_RESPONSES = 1,  // `tg` is read: the (n, R) table, or the gathered (b, k, R) tensor next to prepared tables
  NEED_OUTPUTS = 2,    // `mean` and `var` are written
  KERNEL_IS_GEN = 4,   // the entry serves MGP_KERNEL_MATERN_GEN alone: `kernel_id` is not looked at
  KERNEL_MAY_BE_GEN = 8  // MGP_KERNEL_MATERN_GEN is a known id the entry then refuses itself (MGP_EUNSUPPORTED)
};
enum { ARGS_READY = 1 };  // fused_args: valid arguments and a batch to serve; any other value is the entry's status

// Validates in the order every fused entry has always used -- sizes (MGP_EINVAL), the empty batch (MGP_OK: pointers and
// enum ids are not looked at, outputs may be NULL), then pointers, strides and ids (MGP_EINVAL) -- and fills `a`.
// Checks of one entry alone stay with that entry: in front of the call where they come before the empty-batch return
// (mgp_loocv_*, the smoothness sign of mgp_posterior_gen_*), behind it otherwise.
template <typename T>
int fused_args(FusedArgs& a, int needs, const T* fq, const T* fn, int d, const int64_t* bi, const int64_t* ni, int64_t b,
               int k, const T* tg, int R, int noise_mode, double eps, const T* nd, int kernel_id, int metric_id,
               const T* ls, int ls_count, T* mean, T* var, T* yk, int* info, const void* packed_q = nullptr,
               int64_t q_stride = 0, const void* packed_nn = nullptr, int64_t nn_stride = 0, int targets_batch = 0) {
  if (b < 0 || k < 1 || d < 1 || R < 1) return MGP_EINVAL;
  if (b == 0) return MGP_OK;  // empty shard: nothing to read or write
  if (packed_nn) {
    // both strides cover the features and the 16-byte response slot the gather reads with every row
    const int64_t need = (int64_t)(d * sizeof(T)) + 16;
    if (!packed_q || q_stride < need || nn_stride < need) return MGP_EINVAL;
    // the neighbour table carries the responses, unless they come already gathered (b, k, R)
    if (targets_batch ? tg == nullptr : nn_stride < (int64_t)((d + R) * sizeof(T))) return MGP_EINVAL;
  } else if (!fq || !fn || ((needs & NEED_RESPONSES) && !tg)) {
    return MGP_EINVAL;
  }
  if (!ni || !ls) return MGP_EINVAL;
  if ((needs & NEED_OUTPUTS) && (!mean || !var)) return MGP_EINVAL;
  const bool known_gen = (needs & KERNEL_MAY_BE_GEN) && kernel_id == MGP_KERNEL_MATERN_GEN;
  if (needs & KERNEL_IS_GEN) kernel_id = MGP_KERNEL_MATERN_GEN;
  else if (!valid_kernel(kernel_id) && !known_gen) return MGP_EINVAL;
  if (!valid_metric(metric_id)) return MGP_EINVAL;
  if (noise_mode < MGP_NOISE_SCALAR || noise_mode > MGP_NOISE_BATCH) return MGP_EINVAL;
  if (noise_mode != MGP_NOISE_SCALAR && !nd) return MGP_EINVAL;
  if (ls_count != 1 && ls_count != d) return MGP_EINVAL;
  a = FusedArgs();
  a.feat_q = fq, a.feat_nn = fn, a.batch_idx = bi, a.nn_idx = ni, a.targets = tg, a.targets_batch = targets_batch;
  a.packed_q = packed_q, a.q_stride = q_stride, a.packed_nn = packed_nn, a.nn_stride = nn_stride;
  a.b = b, a.d = d, a.k = k, a.R = R;
  a.noise_mode = noise_mode, a.noise_scalar = eps, a.noise_dev = nd;
  a.kernel_id = kernel_id, a.metric_id = metric_id, a.length_scale = ls, a.ls_count = ls_count;
  a.mean = mean, a.var = var, a.ykinvy = yk, a.info = info;
  return ARGS_READY;
}

template <typename T>
int posterior(const T* fq, const T* fn, int d, const int64_t* bi, const int64_t* ni, int64_t b, int k, const T* tg,
              int R, int noise_mode, double eps, const T* nd, int kernel_id, int metric_id, const T* ls,
              int ls_count, T* mean, T* var, T* yk, int* info, void* stream, int path = PATH_AUTO,
              const void* packed_q = nullptr, int64_t q_stride = 0, const void* packed_nn = nullptr,
              int64_t nn_stride = 0, int targets_batch = 0, const LoocvTree* tree = nullptr, bool* tree_served = nullptr) {
  FusedArgs a;
  const int ready = fused_args<T>(a, NEED_RESPONSES | NEED_OUTPUTS, fq, fn, d, bi, ni, b, k, tg, R, noise_mode, eps, nd,
                                  kernel_id, metric_id, ls, ls_count, mean, var, yk, info, packed_q, q_stride, packed_nn,
                                  nn_stride, targets_batch);
  if (ready != ARGS_READY) return ready;
  const bool packed = packed_nn != nullptr;
  hipStream_t s = static_cast<hipStream_t>(stream);
  // a LOOCV evaluation (mgp_loocv_*): the wave kernels walk the reduction tree themselves (one launch); behind the
  // other families the caller does
  if (tree) a.tree = *tree;
  if (tree_served) *tree_served = false;
  if (packed || path == PATH_AUTO) {
    int rc = launch_fused_wave<T>(a, s);
    if (rc == MGP_OK && tree && tree_served) *tree_served = true;
    if (rc == MGP_EUNSUPPORTED && tree) {  // (a grid beyond the tree's leaves: the plain launch, the tree by kernels)
      a.tree = LoocvTree{};
      rc = launch_fused_wave<T>(a, s);
    }
    // prepared tables with up to sixteen responses behind the features (round 5): the fp32 prediction kernel on the
    // matrix cores' layout reads them too (BASELINE config 5: two 128-byte lines per neighbour instead of three)
    if constexpr (sizeof(T) == 4) {
      if (packed && rc == MGP_EUNSUPPORTED && !tree && !yk) rc = launch_fused_rhs_mf(a, s);
    }
    if (packed || rc != MGP_EUNSUPPORTED) return rc;  // (prepared tables, MGP_EUNSUPPORTED: the caller uses the plain tables)
  }
  a.tree = LoocvTree{};
  if (path == PATH_RHS) return launch_fused_rhs<T>(a, s);
  if (path == PATH_AUTO) {
    int rc;
    rc = launch_fused_rhs<T>(a, s);
    if (rc != MGP_EUNSUPPORTED) return rc;
    rc = launch_fused_wide<T>(a, s);
    if (rc != MGP_EUNSUPPORTED) return rc;
    if constexpr (sizeof(T) == 8) {
      rc = launch_fused_wide64(a, s);
      if (rc != MGP_EUNSUPPORTED) return rc;
    }
  }
  return launch_fused_generic<T>(a, s);
}

// fused fast-mean precompute: coefficients K^-1 y of every neighbourhood (no query involved)
template <typename T>
int fast_coefficients(const T* fn, int d, const int64_t* ni, int64_t b, int k, const T* tg, int noise_mode, double eps,
                      const T* nd, int kernel_id, int metric_id, const T* ls, int ls_count, T* coeffs, int* info,
                      void* stream) {
  FusedArgs a;
  // the query slot is fed the first neighbour of each row: its outputs are not stored
  const int ready = fused_args<T>(a, NEED_RESPONSES, fn, fn, d, nullptr, ni, b, k, tg, 1, noise_mode, eps, nd, kernel_id,
                                  metric_id, ls, ls_count, nullptr, nullptr, nullptr, info);
  if (ready != ARGS_READY) return ready;
  if (!coeffs) return MGP_EINVAL;
  a.coeffs = coeffs;
  return launch_fused_wave<T>(a, static_cast<hipStream_t>(stream));
}

// prediction from precomputed coefficients: no responses, no noise (both are inside `coeffs`)
template <typename T>
int fast_posterior_mean(const T* fq, const T* fn, int d, const int64_t* bi, const int64_t* ni, int64_t b, int k,
                        const T* coeffs, const int64_t* crow, int R, int kernel_id, int metric_id, const T* ls,
                        int ls_count, T* mean, void* stream) {
  FusedArgs a;
  const int ready = fused_args<T>(a, 0, fq, fn, d, bi, ni, b, k, nullptr, R, MGP_NOISE_SCALAR, 0.0, nullptr, kernel_id,
                                  metric_id, ls, ls_count, mean, nullptr, nullptr, nullptr);
  if (ready != ARGS_READY) return ready;
  if (!coeffs || !crow || !mean) return MGP_EINVAL;
  return launch_fast_mean<T>(fq, fn, d, bi, ni, b, k, coeffs, crow, R, kernel_id, metric_id, ls, ls_count, mean,
                             static_cast<hipStream_t>(stream));
}

template <typename T>
int posterior_backward(const T* fq, const T* fn, int d, const int64_t* bi, const int64_t* ni, int64_t b, int k,
                       const T* tg, int R, int noise_mode, double eps, const T* nd, int kernel_id, int metric_id,
                       const T* ls, int ls_count, const T* gmean, const T* gvar, T* gfq, T* gfn, T* gtg, T* gls,
                       T* gnz, int* info, void* stream, const T* gyk = nullptr) {
  BackwardArgs g = BackwardArgs();
  const int ready = fused_args<T>(g.f, NEED_RESPONSES, fq, fn, d, bi, ni, b, k, tg, R, noise_mode, eps, nd, kernel_id,
                                  metric_id, ls, ls_count, nullptr, nullptr, nullptr, info);
  if (ready != ARGS_READY) return ready;
  if (!gmean && !gvar && !gyk) return MGP_EINVAL;
  if (gyk && R != 1) return MGP_EINVAL;  // (the LOOCV losses are defined for one response)
  g.grad_mean = gmean, g.grad_var = gvar, g.grad_yk = gyk;
  g.grad_feat_q = gfq, g.grad_feat_nn = gfn, g.grad_targets = gtg, g.grad_ls = gls, g.grad_noise = gnz;
  static const bool lds_only = getenv("MGP_BACKWARD_LDS") != nullptr;  // A/B switch (timing only)
  // hyper-parameter gradients on the forward kernel itself (round 6: the dealt-triangle shapes of BASELINE config 4 and
  // the 32-slot shapes of config 3)
  if (!lds_only) {
    const int rc = launch_backward_fwd<T>(g, static_cast<hipStream_t>(stream));
    if (rc != MGP_EUNSUPPORTED) return rc;
  }
  if (!lds_only) {
    const int rc = launch_backward_wave<T>(g, static_cast<hipStream_t>(stream));
    if (rc != MGP_EUNSUPPORTED) return rc;
  }
  return launch_backward<T>(g, static_cast<hipStream_t>(stream));
}

// the whole vector-Jacobian product of the general-smoothness Matern in LDS (mgp_backward_gen.hip): the checks of
// hyper_backward_gen_large in its order, without a workspace; gyk selects the LOOCV form, grad_nu is a sixth output
template <typename T>
int posterior_backward_gen(const T* fq, const T* fn, int d, const int64_t* bi, const int64_t* ni, int64_t b, int k,
                           const T* tg, int R, int noise_mode, double eps, const T* nd, double smoothness, int metric_id,
                           const T* ls, int ls_count, const T* gmean, const T* gvar, const T* gyk, T* gfq, T* gfn, T* gtg,
                           T* gls, T* gnz, T* gnu, int* info, void* stream) {
  if (!(smoothness > 0.0)) return MGP_EINVAL;
  BackwardArgs g = BackwardArgs();
  const int ready = fused_args<T>(g.f, NEED_RESPONSES | KERNEL_IS_GEN, fq, fn, d, bi, ni, b, k, tg, R, noise_mode, eps, nd,
                                  MGP_KERNEL_MATERN_GEN, metric_id, ls, ls_count, nullptr, nullptr, nullptr, info);
  if (ready != ARGS_READY) return ready;
  if (gyk && R != 1) return MGP_EINVAL;  // (the LOOCV losses are defined for one response)
  if ((!gmean && !gvar && !gyk) || (!gfq && !gfn && !gtg && !gls && !gnz && !gnu)) return MGP_EINVAL;
  if (smoothness > 30.0) return MGP_EUNSUPPORTED;
  g.f.smoothness = smoothness;
  g.grad_mean = gmean, g.grad_var = gvar, g.grad_yk = gyk;
  g.grad_feat_q = gfq, g.grad_feat_nn = gfn, g.grad_targets = gtg, g.grad_ls = gls, g.grad_noise = gnz;
  return launch_backward_gen<T>(g, gnu, static_cast<hipStream_t>(stream));  // (refuses k beyond max_nn_count_backward_gen)
}

template <typename T>
int solve(const T* Kin, const T* Kc, const T* Y, int64_t b, int k, int R, double kout, T* mean, T* var, T* yk,
          T* coeffs, int* info, void* stream) {
  if (b < 0 || k < 1 || R < 0) return MGP_EINVAL;
  if (b == 0) return MGP_OK;
  if (!Kin) return MGP_EINVAL;
  if (R > 0 && !Y) return MGP_EINVAL;
  if ((mean || var) && !Kc) return MGP_EINVAL;
  if ((mean || yk || coeffs) && R == 0) return MGP_EINVAL;
  if (b == 0) return MGP_OK;
  SolveArgs a{Kin, Kc, Y, mean, var, yk, coeffs, info, b, kout, k, R};
  const int rc = launch_solve_wave<T>(a, static_cast<hipStream_t>(stream));
  if (rc != MGP_EUNSUPPORTED) return rc;
  return launch_solve_generic<T>(a, static_cast<hipStream_t>(stream));
}
// ---- systems beyond LDS (mgp_large.hip) ------------------------------------------------------------------------------
// the workspace of an mgp_*_large_* call: 16-byte aligned, at least one slab (checked with the pointers, before a
// shape beyond the kernel is refused)
static bool valid_workspace(const void* ws, int64_t bytes, int elem_size, int k, int R) {
  return ws && reinterpret_cast<uintptr_t>(ws) % 16 == 0 && bytes >= large_slab_bytes(elem_size, k, R);
}

template <typename T>
int posterior_large(const T* fq, const T* fn, int d, const int64_t* bi, const int64_t* ni, int64_t b, int k, const T* tg,
                    int R, int targets_batch, int noise_mode, double eps, const T* nd, int kernel_id, int metric_id,
                    const T* ls, int ls_count, T* mean, T* var, T* yk, int* info, void* ws, int64_t ws_bytes,
                    void* stream) {
  FusedArgs a;
  const int ready = fused_args<T>(a, NEED_RESPONSES | NEED_OUTPUTS | KERNEL_MAY_BE_GEN, fq, fn, d, bi, ni, b, k, tg, R,
                                  noise_mode, eps, nd, kernel_id, metric_id, ls, ls_count, mean, var, yk, info, nullptr, 0,
                                  nullptr, 0, targets_batch != 0);
  if (ready != ARGS_READY) return ready;
  if (!valid_workspace(ws, ws_bytes, sizeof(T), k, R)) return MGP_EINVAL;
  return launch_fused_large<T>(a, ws, ws_bytes, static_cast<hipStream_t>(stream));  // (refuses rows > 1024 and the general nu)
}

// the fast-mean precompute for any k and response count: the system in LDS up to mgp_max_nn_count (no workspace), on a
// slab of the caller's workspace beyond; the checks in the order of posterior_large
// (a system beyond the slab kernel: its workspace is checked like any other before the shape is refused)
static bool coefficients_need_workspace(int elem_size, int k, int R) {
  return (int64_t)k + 1 + R > kLargeMaxRows || k > max_nn_count(elem_size, R);
}

template <typename T>
int fast_coefficients_any(const T* fn, int d, const int64_t* ni, int64_t b, int k, const T* tg, int R, int noise_mode,
                          double eps, const T* nd, int kernel_id, int metric_id, const T* ls, int ls_count, T* coeffs,
                          int* info, void* ws, int64_t ws_bytes, void* stream) {
  FusedArgs a;
  const int ready = fused_args<T>(a, NEED_RESPONSES | KERNEL_MAY_BE_GEN, fn, fn, d, nullptr, ni, b, k, tg, R, noise_mode, eps,
                                  nd, kernel_id, metric_id, ls, ls_count, nullptr, nullptr, nullptr, info);
  if (ready != ARGS_READY) return ready;
  if (!coeffs) return MGP_EINVAL;
  const bool large = coefficients_need_workspace(sizeof(T), k, R);
  if (large && !valid_workspace(ws, ws_bytes, sizeof(T), k, R)) return MGP_EINVAL;
  if ((int64_t)k + 1 + R > kLargeMaxRows || kernel_id == MGP_KERNEL_MATERN_GEN) return MGP_EUNSUPPORTED;
  a.coeffs = coeffs;
  hipStream_t s = static_cast<hipStream_t>(stream);
  return large ? launch_fused_large<T>(a, ws, ws_bytes, s) : launch_fused_generic<T>(a, s);
}

// ... of the general-smoothness Matern (mgp_fast_coefficients_gen_*): the GEN x COEFFS instantiations of the same two
// families, the LDS limit with the node table in place (mgp_max_nn_count_gen); the checks of fast_coefficients_any in
// its order, the smoothness sign with the sizes (in front of the empty-batch return), its limit with the shapes beyond
// the kernels
static bool coefficients_gen_need_workspace(int elem_size, int k, int R) {
  return (int64_t)k + 1 + R > kLargeMaxRows || k > max_nn_count_gen(elem_size, R);
}

template <typename T>
int fast_coefficients_gen(const T* fn, int d, const int64_t* ni, int64_t b, int k, const T* tg, int R, int noise_mode,
                          double eps, const T* nd, double smoothness, int metric_id, const T* ls, int ls_count, T* coeffs,
                          int* info, void* ws, int64_t ws_bytes, void* stream) {
  if (!(smoothness > 0.0)) return MGP_EINVAL;
  FusedArgs a;
  const int ready = fused_args<T>(a, NEED_RESPONSES | KERNEL_IS_GEN, fn, fn, d, nullptr, ni, b, k, tg, R, noise_mode, eps, nd,
                                  MGP_KERNEL_MATERN_GEN, metric_id, ls, ls_count, nullptr, nullptr, nullptr, info);
  if (ready != ARGS_READY) return ready;
  if (!coeffs) return MGP_EINVAL;
  const bool large = coefficients_gen_need_workspace(sizeof(T), k, R);
  if (large && !valid_workspace(ws, ws_bytes, sizeof(T), k, R)) return MGP_EINVAL;
  if ((int64_t)k + 1 + R > kLargeMaxRows || smoothness > 30.0) return MGP_EUNSUPPORTED;
  a.coeffs = coeffs;
  a.smoothness = smoothness;
  hipStream_t s = static_cast<hipStream_t>(stream);
  return large ? launch_fused_large_gen<T>(a, ws, ws_bytes, s) : launch_fused_generic_gen<T>(a, s);
}

// ... and the prediction from such coefficients (mgp_fast_posterior_mean_gen_*): the checks of fast_posterior_mean, the
// smoothness as above; a list of more than 1023 neighbours is refused (no coefficient entry writes one: k + 1 + R <=
// 1024, and up to there the covariances of a test point and the fp64 node table fit the default 64 KiB of dynamic LDS)
template <typename T>
int fast_posterior_mean_gen(const T* fq, const T* fn, int d, const int64_t* bi, const int64_t* ni, int64_t b, int k,
                            const T* coeffs, const int64_t* crow, int R, double smoothness, int metric_id, const T* ls,
                            int ls_count, T* mean, void* stream) {
  if (!(smoothness > 0.0)) return MGP_EINVAL;
  FusedArgs a;
  const int ready = fused_args<T>(a, KERNEL_IS_GEN, fq, fn, d, bi, ni, b, k, nullptr, R, MGP_NOISE_SCALAR, 0.0, nullptr,
                                  MGP_KERNEL_MATERN_GEN, metric_id, ls, ls_count, mean, nullptr, nullptr, nullptr);
  if (ready != ARGS_READY) return ready;
  if (!coeffs || !crow || !mean) return MGP_EINVAL;
  if ((int64_t)k + 1 > kLargeMaxRows || smoothness > 30.0) return MGP_EUNSUPPORTED;
  return launch_fast_mean_gen<T>(fq, fn, d, bi, ni, b, k, coeffs, crow, R, smoothness, metric_id, ls, ls_count, mean,
                                 static_cast<hipStream_t>(stream));
}

template <typename T>
int solve_large(const T* Kin, const T* Kc, const T* Y, int64_t b, int k, int R, double kout, T* mean, T* var, T* yk,
                T* coeffs, int* info, void* ws, int64_t ws_bytes, void* stream) {
  if (b < 0 || k < 1 || R < 0) return MGP_EINVAL;
  if (b == 0) return MGP_OK;
  if (!Kin) return MGP_EINVAL;
  if (R > 0 && !Y) return MGP_EINVAL;
  if ((mean || var) && !Kc) return MGP_EINVAL;
  if ((mean || yk || coeffs) && R == 0) return MGP_EINVAL;
  if (!valid_workspace(ws, ws_bytes, sizeof(T), k, R)) return MGP_EINVAL;
  SolveArgs a{Kin, Kc, Y, mean, var, yk, coeffs, info, b, kout, k, R};
  return launch_solve_large<T>(a, ws, ws_bytes, static_cast<hipStream_t>(stream));
}

// the hyper-parameter backward on the slab factor (mgp_backward_large.hip): one table on both sides
template <typename T>
int hyper_backward_large(const T* feat, int d, const int64_t* bi, const int64_t* ni, int64_t b, int k, const T* tg, int R,
                         int noise_mode, double eps, const T* nd, int kernel_id, int metric_id, const T* ls, int ls_count,
                         const T* gmean, const T* gvar, const T* gyk, T* gls, T* gnz, int* info, void* ws,
                         int64_t ws_bytes, void* stream) {
  BackwardArgs g = BackwardArgs();
  const int ready = fused_args<T>(g.f, NEED_RESPONSES | KERNEL_MAY_BE_GEN, feat, feat, d, bi, ni, b, k, tg, R, noise_mode,
                                  eps, nd, kernel_id, metric_id, ls, ls_count, nullptr, nullptr, nullptr, info);
  if (ready != ARGS_READY) return ready;
  if (gyk && R != 1) return MGP_EINVAL;  // (the LOOCV losses are defined for one response)
  if ((!gmean && !gvar && !gyk) || (!gls && !gnz)) return MGP_EINVAL;
  if (!ws || reinterpret_cast<uintptr_t>(ws) % 16 != 0 || ws_bytes < backward_large_slab_bytes(sizeof(T), k))
    return MGP_EINVAL;
  g.grad_mean = gmean, g.grad_var = gvar, g.grad_yk = gyk, g.grad_ls = gls, g.grad_noise = gnz;
  return launch_hyper_backward_large<T>(g, ws, ws_bytes, static_cast<hipStream_t>(stream));  // (refuses k + 2 > 1024 and the general nu)
}

// ... of the general-smoothness Matern (mgp_backward_gen_large.hip): the same checks in the same order, the smoothness
// sign with the sizes (in front of the empty-batch return), its limit with the shapes beyond the kernel; grad_nu is a
// third output
template <typename T>
int hyper_backward_gen_large(const T* feat, int d, const int64_t* bi, const int64_t* ni, int64_t b, int k, const T* tg,
                             int R, int noise_mode, double eps, const T* nd, double smoothness, int metric_id, const T* ls,
                             int ls_count, const T* gmean, const T* gvar, const T* gyk, T* gls, T* gnz, T* gnu, int* info,
                             void* ws, int64_t ws_bytes, void* stream) {
  if (!(smoothness > 0.0)) return MGP_EINVAL;
  BackwardArgs g = BackwardArgs();
  const int ready = fused_args<T>(g.f, NEED_RESPONSES | KERNEL_IS_GEN, feat, feat, d, bi, ni, b, k, tg, R, noise_mode, eps,
                                  nd, MGP_KERNEL_MATERN_GEN, metric_id, ls, ls_count, nullptr, nullptr, nullptr, info);
  if (ready != ARGS_READY) return ready;
  if (gyk && R != 1) return MGP_EINVAL;  // (the LOOCV losses are defined for one response)
  if ((!gmean && !gvar && !gyk) || (!gls && !gnz && !gnu)) return MGP_EINVAL;
  if (!ws || reinterpret_cast<uintptr_t>(ws) % 16 != 0 || ws_bytes < backward_large_slab_bytes(sizeof(T), k))
    return MGP_EINVAL;
  if (smoothness > 30.0) return MGP_EUNSUPPORTED;
  g.f.smoothness = smoothness;
  g.grad_mean = gmean, g.grad_var = gvar, g.grad_yk = gyk, g.grad_ls = gls, g.grad_noise = gnz;
  return launch_hyper_backward_gen_large<T>(g, gnu, ws, ws_bytes, static_cast<hipStream_t>(stream));  // (refuses k + 2 > 1024)
}

// ... and the whole vector-Jacobian product there: two tables, every cotangent of mgp_posterior_backward_*
template <typename T>
int posterior_backward_large(const T* fq, const T* fn, int d, const int64_t* bi, const int64_t* ni, int64_t b, int k,
                             const T* tg, int R, int noise_mode, double eps, const T* nd, int kernel_id, int metric_id,
                             const T* ls, int ls_count, const T* gmean, const T* gvar, T* gfq, T* gfn, T* gtg, T* gls,
                             T* gnz, int* info, void* ws, int64_t ws_bytes, void* stream) {
  BackwardArgs g = BackwardArgs();
  const int ready = fused_args<T>(g.f, NEED_RESPONSES | KERNEL_MAY_BE_GEN, fq, fn, d, bi, ni, b, k, tg, R, noise_mode, eps,
                                  nd, kernel_id, metric_id, ls, ls_count, nullptr, nullptr, nullptr, info);
  if (ready != ARGS_READY) return ready;
  if ((!gmean && !gvar) || (!gfq && !gfn && !gtg && !gls && !gnz)) return MGP_EINVAL;
  if (!ws || reinterpret_cast<uintptr_t>(ws) % 16 != 0 || ws_bytes < backward_large_slab_bytes(sizeof(T), k))
    return MGP_EINVAL;
  g.grad_mean = gmean, g.grad_var = gvar;
  g.grad_feat_q = gfq, g.grad_feat_nn = gfn, g.grad_targets = gtg, g.grad_ls = gls, g.grad_noise = gnz;
  return launch_posterior_backward_large<T>(g, ws, ws_bytes, static_cast<hipStream_t>(stream));  // (refuses k + 2 > 1024 and the general nu)
}

// behind the fused launch of a LOOCV evaluation: nothing when a wave kernel walked the tree itself; the walk by kernels
// over the SAME leaves when it was launched without (three_launch); over the canonical leaves behind another family
template <typename T>
int loocv_finish(int rc, bool served, const LoocvTree& tr, const T* mean, const T* var, const T* yk, const int64_t* bi,
                 int64_t b, hipStream_t s) {
  if (rc != MGP_OK) return rc;
  if (served && tr.mode != kTreeThreeLaunch) return MGP_OK;
  const int grid = served ? g_tree_grid : 0, nh = served ? g_tree_nh : 0;
  return launch_loocv_tree<T>(tr, grid, nh, mean, var, yk, bi, b, s);
}
}  // namespace mgp

using namespace mgp;
#define S_(x) static_cast<hipStream_t>(x)

// General-smoothness Matern, evaluated inside the fused launch.  Up to 64 slots (k + 1 + R): the wave kernels (fp32:
// k + 1 + R <= 32 or a static shape; fp64: the static shapes) or MGP_EUNSUPPORTED, on either table form.  Beyond 64
// slots, plain tables: the general-smoothness instantiation of the LDS workgroup kernel (mgp_generic.hip) wherever it
// fits LDS with its node table; MGP_EUNSUPPORTED where it does not (the caller goes on to mgp_posterior_gen_large_*)
// and for prepared tables.  Where everything refuses the caller evaluates mgp_matern_gen_* on materialised distances.
template <typename T>
static int posterior_gen(const T* fq, const T* fn, const void* packed_q, int64_t q_stride, const void* packed_nn,
                         int64_t nn_stride, int d, const int64_t* bi, const int64_t* ni, int64_t b, int k, const T* tg,
                         int R, int targets_batch, int noise_mode, double eps, const T* nd, double smoothness,
                         int metric_id, const T* ls, int ls_count, T* mean, T* var, T* yk, int* info, void* stream,
                         int path = PATH_AUTO) {
  if (!(smoothness > 0.0)) return MGP_EINVAL;  // (in front of the empty-batch return, like the sizes)
  FusedArgs a;
  const int ready = fused_args<T>(a, NEED_RESPONSES | NEED_OUTPUTS | KERNEL_IS_GEN, fq, fn, d, bi, ni, b, k, tg, R,
                                  noise_mode, eps, nd, MGP_KERNEL_MATERN_GEN, metric_id, ls, ls_count, mean, var, yk,
                                  info, packed_q, q_stride, packed_nn, nn_stride, targets_batch);
  if (ready != ARGS_READY) return ready;
  if (smoothness > 30.0) return MGP_EUNSUPPORTED;  // beyond nu = 30 the RBF limit is the better model anyway
  a.smoothness = smoothness;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (path == PATH_GENERIC) return launch_fused_generic_gen<T>(a, s);  // (mgp_posterior_gen_generic_*: the family by name)
  // (beyond their 64 slots the wave kernels refuse every shape: on the plain tables the LDS workgroup kernel is next)
  if (packed_nn || (int64_t)k + 1 + R <= 64) return launch_fused_wave<T>(a, s);
  return launch_fused_generic_gen<T>(a, s);
}

// ... and on the slab factor beyond LDS (mgp_large.hip): the checks of posterior_large, then the smoothness limit
template <typename T>
static int posterior_gen_large(const T* fq, const T* fn, int d, const int64_t* bi, const int64_t* ni, int64_t b, int k,
                               const T* tg, int R, int targets_batch, int noise_mode, double eps, const T* nd,
                               double smoothness, int metric_id, const T* ls, int ls_count, T* mean, T* var, T* yk,
                               int* info, void* ws, int64_t ws_bytes, void* stream) {
  if (!(smoothness > 0.0)) return MGP_EINVAL;
  FusedArgs a;
  const int ready = fused_args<T>(a, NEED_RESPONSES | NEED_OUTPUTS | KERNEL_IS_GEN, fq, fn, d, bi, ni, b, k, tg, R,
                                  noise_mode, eps, nd, MGP_KERNEL_MATERN_GEN, metric_id, ls, ls_count, mean, var, yk,
                                  info, nullptr, 0, nullptr, 0, targets_batch != 0);
  if (ready != ARGS_READY) return ready;
  if (!valid_workspace(ws, ws_bytes, sizeof(T), k, R)) return MGP_EINVAL;
  if (smoothness > 30.0) return MGP_EUNSUPPORTED;
  a.smoothness = smoothness;
  return launch_fused_large_gen<T>(a, ws, ws_bytes, static_cast<hipStream_t>(stream));  // (refuses rows > 1024)
}

// A length scale per neighbourhood (mgp_posterior_ns_*): the NS instantiations of the two workgroup families by name.
// The checks of posterior_gen (PATH_GENERIC) / posterior_gen_large in their order, `lsb` (b, ls_count) in the place of
// the launch's length scale(s); the general smoothness is a known id both refuse.
template <typename T>
static int posterior_ns(const T* fq, const T* fn, int d, const int64_t* bi, const int64_t* ni, int64_t b, int k, const T* tg,
                        int R, int targets_batch, int noise_mode, double eps, const T* nd, int kernel_id, int metric_id,
                        const T* lsb, int ls_count, T* mean, T* var, T* yk, int* info, void* stream) {
  FusedArgs a;
  const int ready = fused_args<T>(a, NEED_RESPONSES | NEED_OUTPUTS | KERNEL_MAY_BE_GEN, fq, fn, d, bi, ni, b, k, tg, R,
                                  noise_mode, eps, nd, kernel_id, metric_id, lsb, ls_count, mean, var, yk, info, nullptr, 0,
                                  nullptr, 0, targets_batch != 0);
  if (ready != ARGS_READY) return ready;
  if (kernel_id == MGP_KERNEL_MATERN_GEN) return MGP_EUNSUPPORTED;
  return launch_fused_generic_ns<T>(a, lsb, static_cast<hipStream_t>(stream));  // (refuses a system beyond LDS)
}
template <typename T>
static int posterior_ns_large(const T* fq, const T* fn, int d, const int64_t* bi, const int64_t* ni, int64_t b, int k,
                              const T* tg, int R, int targets_batch, int noise_mode, double eps, const T* nd, int kernel_id,
                              int metric_id, const T* lsb, int ls_count, T* mean, T* var, T* yk, int* info, void* ws,
                              int64_t ws_bytes, void* stream) {
  FusedArgs a;
  const int ready = fused_args<T>(a, NEED_RESPONSES | NEED_OUTPUTS | KERNEL_MAY_BE_GEN, fq, fn, d, bi, ni, b, k, tg, R,
                                  noise_mode, eps, nd, kernel_id, metric_id, lsb, ls_count, mean, var, yk, info, nullptr, 0,
                                  nullptr, 0, targets_batch != 0);
  if (ready != ARGS_READY) return ready;
  if (!valid_workspace(ws, ws_bytes, sizeof(T), k, R)) return MGP_EINVAL;
  return launch_fused_large_ns<T>(a, lsb, ws, ws_bytes, static_cast<hipStream_t>(stream));  // (refuses rows > 1024 and the general nu)
}

template <typename T>
static int shear_tensor(const T* diffs, int64_t G, int n, int m, int variant, double ls, T* out, void* stream) {
  if (G < 0 || n < 0 || m < 0 || !(ls > 0.0)) return MGP_EINVAL;
  if (variant < MGP_SHEAR_33 || variant > MGP_SHEAR_KCROSS23) return MGP_EINVAL;
  if (G == 0 || n == 0 || m == 0) return MGP_OK;
  if (!diffs || !out) return MGP_EINVAL;
  return launch_shear_tensor<T>(diffs, G, n, m, variant, ls, out, S_(stream));
}
template <typename T>
static int solve_multi(const T* Kin, const T* Kc, const T* Y, int64_t b, int n, int m, int R, T* mean, T* kk, T* yk,
                       int* info, void* stream) {
  if (b < 0 || n < 1 || m < 1 || R < 0) return MGP_EINVAL;
  if (!Kin || !Kc || (R > 0 && !Y) || ((mean || yk) && R == 0) || (!mean && !kk && !yk)) return MGP_EINVAL;
  if (b == 0) return MGP_OK;
  SolveMultiArgs a{Kin, Kc, Y, mean, kk, yk, info, b, n, m, R};
  return launch_solve_multi<T>(a, S_(stream));
}
template <typename T>
static int shear_posterior(const T* fq, const T* fn, const int64_t* bi, const int64_t* ni, int64_t b, int k, int in,
                           const T* tg, int64_t tstride, int tbatch, double ls, int noise_mode, double noise, T* mean,
                           T* kk, T* yk, int* info, void* stream) {
  if (b < 0 || k < 1 || (in != 2 && in != 3) || !(ls > 0.0) || !(noise >= 0.0)) return MGP_EINVAL;
  if (noise_mode != MGP_SHEAR_NOISE_HOMOSCEDASTIC && noise_mode != MGP_SHEAR_NOISE_33) return MGP_EINVAL;
  if (noise_mode == MGP_SHEAR_NOISE_33 && in != 3) return MGP_EINVAL;
  if (!fq || !fn || !ni || !tg || !mean || !kk) return MGP_EINVAL;
  if (!tbatch && tstride < in) return MGP_EINVAL;
  if (b == 0) return MGP_OK;  // (launch_shear_posterior refuses a k beyond the LDS before any HIP call)
  ShearArgs a{fq, fn, bi, ni, tg, tstride, tbatch, mean, kk, yk, info, b, ls, noise, k, in, noise_mode};
  return launch_shear_posterior<T>(a, S_(stream));
}

extern "C" {

const char* mgp_version(void) { return "muygpys_amd-hip 0.1 (gfx950)"; }
int mgp_max_nn_count(int elem_size, int R) { return max_nn_count(elem_size, R); }
int mgp_max_nn_count_gen(int elem_size, int R) {
  if ((elem_size != 4 && elem_size != 8) || R < 0) return MGP_EINVAL;
  return max_nn_count_gen(elem_size, R);
}
int mgp_reduce_scratch_doubles(void) { return reduce_scratch_doubles(); }
int64_t mgp_loocv_scratch_bytes(void) { return tree_scratch_bytes(); }
int64_t mgp_loocv_scratch_zero_bytes(void) { return tree_zero_bytes(); }
int mgp_last_launch_geometry(int64_t* workgroups, int* lds_bytes) {
  if (!workgroups || !lds_bytes) return MGP_EINVAL;
  *workgroups = g_launch_grid, *lds_bytes = g_launch_lds;
  return MGP_OK;
}
int mgp_loocv_tree_mode_get(void) { return g_tree_mode; }
int mgp_loocv_tree_mode_set(int mode) {
  if (mode != kTreeTickets && mode != kTreeFenced && mode != kTreeThreeLaunch) return MGP_EINVAL;
  g_tree_mode = mode;
  return MGP_OK;
}
int mgp_last_loocv_geometry(int* grid, int* nh) {
  if (!grid || !nh) return MGP_EINVAL;
  *grid = g_tree_grid, *nh = g_tree_nh;
  return MGP_OK;
}
int mgp_matern_gen_constants(double smoothness, double* out7) {
  if (!out7 || !(smoothness > 0.0)) return MGP_EINVAL;
  matern_gen_constants_host(smoothness, out7);
  return MGP_OK;
}
int mgp_posterior_kernel_name(int elem_size, int d, int k, int R, int packed, int path, char* buf, int len) {
  if (!buf || len < 1 || (elem_size != 4 && elem_size != 8)) return MGP_EINVAL;
  if (path == PATH_AUTO && describe_fused_wave(elem_size, d, k, R, packed, buf, len) > 0) return MGP_OK;
  const char* t = elem_size == 4 ? "float" : "double";
  if (packed) return snprintf(buf, len, "%s", "") < 0 ? MGP_EINVAL : MGP_EUNSUPPORTED;
  if (path != PATH_GENERIC && k <= 64 && R <= 16)
    snprintf(buf, len, "mgp::fused_rhs_kernel<%s,%d>", t, R <= 4 ? 4 : 16);
  else if (path == PATH_AUTO && k + 1 + R >= 65 && k + 1 + R <= 128 && R <= 16 && d <= 64)
    snprintf(buf, len, elem_size == 4 ? "mgp::fused_wide_kernel" : "mgp::fused_wide64_kernel");
  else
    snprintf(buf, len, "mgp::fused_generic_kernel<%s>", t);
  return MGP_OK;
}
int mgp_shear_max_nn_count(int elem_size, int in_count) {
  if ((elem_size != 4 && elem_size != 8) || (in_count != 2 && in_count != 3)) return MGP_EINVAL;
  return shear_max_nn_count(elem_size, in_count);
}
int mgp_last_kernel_name(char* buf, int len) {
  if (!buf || len < 1) return MGP_EINVAL;
  snprintf(buf, len, "%s", mgp::g_last_kernel);
  return MGP_OK;
}
int mgp_allreduce_partials(double* partials, int count, void* nccl_comm, void* st) {
  return allreduce_partials(partials, count, nccl_comm, S_(st));
}
int mgp_jit_prepare(int elem_size, int k, int R, int d, int packed, int kernel_id) {
  if ((elem_size != 4 && elem_size != 8) || k < 1 || R < 1 || d < 1 || !(valid_kernel(kernel_id) || kernel_id == MGP_KERNEL_MATERN_GEN))
    return MGP_EINVAL;
  return prepare_fused_wave(elem_size, d, k, R, packed, kernel_id);
}
int mgp_jit_prepare_backward(int elem_size, int k, int d, int kernel_id) {
  if ((elem_size != 4 && elem_size != 8) || k < 1 || d < 1 || !valid_kernel(kernel_id)) return MGP_EINVAL;
  return prepare_backward_fwd(elem_size, k, d, kernel_id);
}
int mgp_jit_mode(void) { return jit_mode(); }
int mgp_jit_loaded_count(void) { return jit_loaded_count(); }
int mgp_jit_source_hash(char* buf, int len) {
  if (!buf || len < 17) return MGP_EINVAL;
  snprintf(buf, len, "%016llx", (unsigned long long)jit_source_hash());
  return MGP_OK;
}
int64_t mgp_packed_row_bytes(int d, int R, int elem_size) {
  if (d < 1 || R < 0 || (elem_size != 4 && elem_size != 8)) return MGP_EINVAL;
  // the gather always reads the 16-byte slot behind the features (the responses), also from a table
  // packed without responses (a query table): the stride reserves it, so the read stays inside the row
  const int64_t resp = (int64_t)R * elem_size > 16 ? (int64_t)R * elem_size : 16;
  return ((int64_t)d * elem_size + resp + 63) / 64 * 64;
}
#ifdef MGP_DEBUG_HOOKS
/* timing-ablation hooks of debug builds (tools/kbench.py, tools/bwdbench.py); absent from the shipped library */
void mgp_debug_set_phase_mask(int mask) { mgp::g_phase_mask = mask; }
void mgp_debug_set_grid_per_cu(int n) { mgp::g_grid_per_cu = n; }
void mgp_debug_set_lds_pad(int n) { mgp::g_lds_pad = n; }
void mgp_debug_set_bwd_stage(int n) { mgp::g_bwd_stage = n; }
#endif

int mgp_posterior_f32(const float* fq, const float* fn, int d, const int64_t* bi, const int64_t* ni, int64_t b, int k,
                      const float* tg, int R, int nm, double eps, const float* nd, int kid, int mid, const float* ls,
                      int lsc, float* mean, float* var, float* yk, int* info, void* st) {
  return posterior<float>(fq, fn, d, bi, ni, b, k, tg, R, nm, eps, nd, kid, mid, ls, lsc, mean, var, yk, info, st);
}
int mgp_posterior_f64(const double* fq, const double* fn, int d, const int64_t* bi, const int64_t* ni, int64_t b,
                      int k, const double* tg, int R, int nm, double eps, const double* nd, int kid, int mid,
                      const double* ls, int lsc, double* mean, double* var, double* yk, int* info, void* st) {
  return posterior<double>(fq, fn, d, bi, ni, b, k, tg, R, nm, eps, nd, kid, mid, ls, lsc, mean, var, yk, info, st);
}

#define MGP_DEFINE_PATHS(SUF, T)                                                                                    \
  int mgp_posterior_generic_##SUF(const T* fq, const T* fn, int d, const int64_t* bi, const int64_t* ni, int64_t b,  \
                                  int k, const T* tg, int R, int nm, double eps, const T* nd, int kid, int mid,      \
                                  const T* ls, int lsc, T* mean, T* var, T* yk, int* info, void* st) {               \
    return posterior<T>(fq, fn, d, bi, ni, b, k, tg, R, nm, eps, nd, kid, mid, ls, lsc, mean, var, yk, info, st,    \
                        PATH_GENERIC);                                                                               \
  }                                                                                                                  \
  int mgp_posterior_rhs_##SUF(const T* fq, const T* fn, int d, const int64_t* bi, const int64_t* ni, int64_t b,      \
                              int k, const T* tg, int R, int nm, double eps, const T* nd, int kid, int mid,          \
                              const T* ls, int lsc, T* mean, T* var, T* yk, int* info, void* st) {                   \
    return posterior<T>(fq, fn, d, bi, ni, b, k, tg, R, nm, eps, nd, kid, mid, ls, lsc, mean, var, yk, info, st,    \
                        PATH_RHS);                                                                                   \
  }                                                                                                                  \
  int mgp_posterior_gathered_##SUF(const T* fq, const T* fn, int d, const int64_t* bi, const int64_t* ni, int64_t b, \
                                   int k, const T* nn_tg, int R, int nm, double eps, const T* nd, int kid, int mid,  \
                                   const T* ls, int lsc, T* mean, T* var, T* yk, int* info, void* st) {              \
    return posterior<T>(fq, fn, d, bi, ni, b, k, nn_tg, R, nm, eps, nd, kid, mid, ls, lsc, mean, var, yk, info, st, \
                        PATH_AUTO, nullptr, 0, nullptr, 0, 1);                                                       \
  }                                                                                                                  \
  int mgp_table_pack_##SUF(const T* feat, const T* targets, int64_t n, int d, int R, void* packed,                   \
                           int64_t stride_bytes, void* st) {                                                         \
    if (!feat || !packed || n < 0 || d < 1 || R < 0) return MGP_EINVAL;                                              \
    return launch_table_pack<T>(feat, targets, n, d, R, packed, stride_bytes, S_(st));                               \
  }                                                                                                                  \
  int mgp_posterior_packed_##SUF(const void* packed_q, int64_t q_stride, const void* packed_nn, int64_t nn_stride,   \
                                 int d, const int64_t* bi, const int64_t* ni, int64_t b, int k, int R, int nm,       \
                                 double eps, const T* nd, int kid, int mid, const T* ls, int lsc, T* mean, T* var,   \
                                 T* yk, int* info, void* st) {                                                       \
    return posterior<T>(nullptr, nullptr, d, bi, ni, b, k, nullptr, R, nm, eps, nd, kid, mid, ls, lsc, mean, var,   \
                        yk, info, st, PATH_AUTO, packed_q, q_stride, packed_nn, nn_stride);                          \
  }                                                                                                                  \
  int mgp_posterior_packed_gathered_##SUF(const void* packed_q, int64_t q_stride, const void* packed_nn,            \
                                          int64_t nn_stride, int d, const int64_t* bi, const int64_t* ni, int64_t b, \
                                          int k, const T* nn_tg, int R, int nm, double eps, const T* nd, int kid,    \
                                          int mid, const T* ls, int lsc, T* mean, T* var, T* yk, int* info,          \
                                          void* st) {                                                                \
    return posterior<T>(nullptr, nullptr, d, bi, ni, b, k, nn_tg, R, nm, eps, nd, kid, mid, ls, lsc, mean, var, yk, \
                        info, st, PATH_AUTO, packed_q, q_stride, packed_nn, nn_stride, 1);                           \
  }                                                                                                                  \
  int mgp_posterior_gen_##SUF(const T* fq, const T* fn, const void* packed_q, int64_t q_stride,                     \
                              const void* packed_nn, int64_t nn_stride, int d, const int64_t* bi, const int64_t* ni, \
                              int64_t b, int k, const T* tg, int R, int targets_batch, int nm, double eps,          \
                              const T* nd, double smoothness, int mid, const T* ls, int lsc, T* mean, T* var,       \
                              T* yk, int* info, void* st) {                                                          \
    return posterior_gen<T>(fq, fn, packed_q, q_stride, packed_nn, nn_stride, d, bi, ni, b, k, tg, R, targets_batch, \
                            nm, eps, nd, smoothness, mid, ls, lsc, mean, var, yk, info, st);                         \
  }                                                                                                                  \
  int mgp_posterior_gen_generic_##SUF(const T* fq, const T* fn, int d, const int64_t* bi, const int64_t* ni,         \
                                      int64_t b, int k, const T* tg, int R, int targets_batch, int nm, double eps,   \
                                      const T* nd, double smoothness, int mid, const T* ls, int lsc, T* mean,        \
                                      T* var, T* yk, int* info, void* st) {                                          \
    return posterior_gen<T>(fq, fn, nullptr, 0, nullptr, 0, d, bi, ni, b, k, tg, R, targets_batch != 0, nm, eps, nd, \
                            smoothness, mid, ls, lsc, mean, var, yk, info, st, PATH_GENERIC);                        \
  }                                                                                                                  \
  int mgp_posterior_gen_large_##SUF(const T* fq, const T* fn, int d, const int64_t* bi, const int64_t* ni,           \
                                    int64_t b, int k, const T* tg, int R, int targets_batch, int nm, double eps,     \
                                    const T* nd, double smoothness, int mid, const T* ls, int lsc, T* mean, T* var,  \
                                    T* yk, int* info, void* workspace, int64_t workspace_bytes, void* st) {          \
    return posterior_gen_large<T>(fq, fn, d, bi, ni, b, k, tg, R, targets_batch, nm, eps, nd, smoothness, mid, ls,   \
                                  lsc, mean, var, yk, info, workspace, workspace_bytes, st);                         \
  }                                                                                                                  \
  int mgp_loocv_##SUF(const T* feat, int d, const int64_t* bi, const int64_t* ni, int64_t b, int k, const T* tg,     \
                      int nm, double eps, const T* nd, int kid, int mid, const T* ls, int lsc, T* mean, T* var,      \
                      T* yk, int* info, double huber_delta, double* partials, void* scratch, void* st) {             \
    if ((b > 0 && (!mean || !var || !yk)) || !partials || !scratch || !(huber_delta > 0)) return MGP_EINVAL;         \
    LoocvTree tr = loocv_tree_layout(scratch, partials, tg, (int64_t)sizeof(T), huber_delta);                        \
    tr.mode = g_tree_mode;                                                                                           \
    bool served = false;                                                                                             \
    note_tree_geometry(0, 0);                                                                                        \
    const int rc = posterior<T>(feat, feat, d, bi, ni, b, k, tg, 1, nm, eps, nd, kid, mid, ls, lsc, mean, var, yk,  \
                                info, st, PATH_AUTO, nullptr, 0, nullptr, 0, 0, &tr, &served);                       \
    return loocv_finish<T>(rc, served, tr, mean, var, yk, bi, b, S_(st));                                            \
  }                                                                                                                  \
  int mgp_loocv_tree_##SUF(const T* mean, const T* var, const T* yk, const void* resp, int64_t resp_stride,          \
                           const int64_t* bi, int64_t b, double huber_delta, int grid, int nh, double* partials,     \
                           void* scratch, void* st) {                                                                \
    if (b < 0 || (b > 0 && (!mean || !var || !yk || !resp)) || !partials || !scratch || !(huber_delta > 0))          \
      return MGP_EINVAL;                                                                                             \
    return launch_loocv_tree<T>(loocv_tree_layout(scratch, partials, resp, resp_stride, huber_delta), grid, nh,      \
                                mean, var, yk, bi, b, S_(st));                                                       \
  }                                                                                                                  \
  int mgp_loocv_packed_##SUF(const void* packed, int64_t stride, int d, const int64_t* bi, const int64_t* ni,        \
                             int64_t b, int k, int nm, double eps, const T* nd, int kid, int mid, const T* ls,       \
                             int lsc, T* mean, T* var, T* yk, int* info, double huber_delta, double* partials,       \
                             void* scratch, void* st) {                                                              \
    if ((b > 0 && (!mean || !var || !yk)) || !partials || !scratch || !(huber_delta > 0)) return MGP_EINVAL;         \
    LoocvTree tr = loocv_tree_layout(scratch, partials, static_cast<const char*>(packed) + (size_t)d * sizeof(T),    \
                                     stride, huber_delta);                                                           \
    tr.mode = g_tree_mode;                                                                                           \
    bool served = false;                                                                                             \
    note_tree_geometry(0, 0);                                                                                        \
    const int rc = posterior<T>(nullptr, nullptr, d, bi, ni, b, k, nullptr, 1, nm, eps, nd, kid, mid, ls, lsc, mean, \
                                var, yk, info, st, PATH_AUTO, packed, stride, packed, stride, 0, &tr, &served);      \
    return loocv_finish<T>(rc, served, tr, mean, var, yk, bi, b, S_(st));                                            \
  }
MGP_DEFINE_PATHS(f32, float)
MGP_DEFINE_PATHS(f64, double)

int mgp_large_max_nn_count(int elem_size, int R) {
  if ((elem_size != 4 && elem_size != 8) || R < 0) return MGP_EINVAL;
  return kLargeMaxRows - 1 - R > 0 ? kLargeMaxRows - 1 - R : 0;
}
int64_t mgp_large_workspace_bytes(int elem_size, int k, int R, int64_t b) {
  if ((elem_size != 4 && elem_size != 8) || k < 1 || R < 0 || b < 0 || (int64_t)k + 1 + R > kLargeMaxRows) return 0;
  return large_workspace_bytes(elem_size, k, R, b);
}
#define MGP_DEFINE_LARGE(SUF, T)                                                                                    \
  int mgp_posterior_large_##SUF(const T* fq, const T* fn, int d, const int64_t* bi, const int64_t* ni, int64_t b,    \
                                int k, const T* tg, int R, int targets_batch, int nm, double eps, const T* nd,       \
                                int kid, int mid, const T* ls, int lsc, T* mean, T* var, T* yk, int* info,           \
                                void* workspace, int64_t workspace_bytes, void* st) {                                \
    return posterior_large<T>(fq, fn, d, bi, ni, b, k, tg, R, targets_batch, nm, eps, nd, kid, mid, ls, lsc, mean,   \
                              var, yk, info, workspace, workspace_bytes, st);                                        \
  }                                                                                                                  \
  int mgp_solve_large_##SUF(const T* Kin, const T* Kc, const T* Y, int64_t b, int k, int R, double kout, T* mean,    \
                            T* var, T* yk, T* coeffs, int* info, void* workspace, int64_t workspace_bytes,           \
                            void* st) {                                                                              \
    return solve_large<T>(Kin, Kc, Y, b, k, R, kout, mean, var, yk, coeffs, info, workspace, workspace_bytes, st);   \
  }
MGP_DEFINE_LARGE(f32, float)
MGP_DEFINE_LARGE(f64, double)

#define MGP_DEFINE_NS(SUF, T)                                                                                       \
  int mgp_posterior_ns_generic_##SUF(const T* fq, const T* fn, int d, const int64_t* bi, const int64_t* ni,          \
                                     int64_t b, int k, const T* tg, int R, int targets_batch, int nm, double eps,    \
                                     const T* nd, int kid, int mid, const T* lsb, int lsc, T* mean, T* var, T* yk,   \
                                     int* info, void* st) {                                                          \
    return posterior_ns<T>(fq, fn, d, bi, ni, b, k, tg, R, targets_batch, nm, eps, nd, kid, mid, lsb, lsc, mean,     \
                           var, yk, info, st);                                                                       \
  }                                                                                                                  \
  int mgp_posterior_ns_large_##SUF(const T* fq, const T* fn, int d, const int64_t* bi, const int64_t* ni,            \
                                   int64_t b, int k, const T* tg, int R, int targets_batch, int nm, double eps,      \
                                   const T* nd, int kid, int mid, const T* lsb, int lsc, T* mean, T* var, T* yk,     \
                                   int* info, void* workspace, int64_t workspace_bytes, void* st) {                  \
    return posterior_ns_large<T>(fq, fn, d, bi, ni, b, k, tg, R, targets_batch, nm, eps, nd, kid, mid, lsb, lsc,     \
                                 mean, var, yk, info, workspace, workspace_bytes, st);                               \
  }
MGP_DEFINE_NS(f32, float)
MGP_DEFINE_NS(f64, double)

int mgp_topk_rows_f32(const float* x, int64_t rows, int cols, int64_t row_stride, int k, float* out_values, int32_t* out_cols,
                      void* st) {
  if (rows < 0 || cols < 1 || k < 1 || row_stride < cols) return MGP_EINVAL;
  if (rows == 0) return MGP_OK;
  if (!x || !out_values || !out_cols) return MGP_EINVAL;
  return launch_topk_rows(x, rows, cols, row_stride, k, out_values, out_cols, S_(st));
}
int mgp_knn_finish_f32(const float* queries, const float* train, int d, const int32_t* candidates, int64_t m, int k,
                       const int64_t* row_map, int64_t* out_idx, float* out_dist, void* st) {
  if (m < 0 || d < 1 || k < 1) return MGP_EINVAL;
  if (m == 0) return MGP_OK;
  if (!queries || !train || !candidates || !out_idx || !out_dist) return MGP_EINVAL;
  return launch_knn_finish(queries, train, d, candidates, m, k, row_map, out_idx, out_dist, S_(st));
}

int mgp_knn_scan_f32(const float* train, const float* train_sqn, int64_t n, int d, const float* queries,
                     const float* query_sqn, const int64_t* self_idx, int64_t m, int k, int64_t start, float* best_d,
                     int32_t* best_i, int32_t* overflow, void* st) {
  if (n < 0 || m < 0 || d < 1 || k < 1 || start < 0) return MGP_EINVAL;
  if (m == 0 || start >= n) return MGP_OK;
  if (!train || !train_sqn || !queries || !query_sqn || !best_d || !best_i || !overflow) return MGP_EINVAL;
  KnnArgs a{train, train_sqn, queries, query_sqn, self_idx, best_d, best_i, overflow, n, m, start, d, k};
  return launch_knn_scan(a, S_(st));
}

int mgp_knn_wide_max_nn_count(void) { return KNN_WIDE_MAX_K; }
int mgp_knn_scan_wide(const float* train, const float* train_sqn, int64_t n, int d, const float* queries,
                      const float* query_sqn, const int64_t* self_idx, int64_t m, int k, int64_t start, float* best_d,
                      int32_t* best_i, int32_t* overflow, void* st) {
  if (n < 0 || m < 0 || d < 1 || k < 1 || start < 0) return MGP_EINVAL;
  if (m == 0 || start >= n) return MGP_OK;
  if (!train || !train_sqn || !queries || !query_sqn || !best_d || !best_i || !overflow) return MGP_EINVAL;
  KnnArgs a{train, train_sqn, queries, query_sqn, self_idx, best_d, best_i, overflow, n, m, start, d, k};
  return launch_knn_scan_wide(a, S_(st));
}
int mgp_knn_finish_wide(const float* queries, const float* train, int d, const int32_t* candidates, int64_t m, int k,
                        const int64_t* row_map, int64_t* out_idx, float* out_dist, void* st) {
  if (m < 0 || d < 1 || k < 1) return MGP_EINVAL;
  if (m == 0) return MGP_OK;
  if (!queries || !train || !candidates || !out_idx || !out_dist) return MGP_EINVAL;
  return launch_knn_finish_wide(queries, train, d, candidates, m, k, row_map, out_idx, out_dist, S_(st));
}

int mgp_knn_scan_bf16x3(const float* train, const void* packed_train, const float* train_sqn, int64_t n, int d,
                        const float* queries, const void* packed_queries, const float* query_sqn,
                        const int64_t* self_idx, int64_t m, int k, int64_t start, float* best_d, int32_t* best_i,
                        int32_t* overflow, void* st) {
  if (n < 0 || m < 0 || d < 1 || k < 1 || start < 0) return MGP_EINVAL;
  if (m == 0 || start >= n) return MGP_OK;
  if (!train || !packed_train || !train_sqn || !queries || !packed_queries || !query_sqn || !best_d || !best_i ||
      !overflow)
    return MGP_EINVAL;
  KnnPackedArgs a{train, packed_train, train_sqn, queries, packed_queries, query_sqn, self_idx, best_d, best_i,
                  overflow, n, m, start, d, k};
  return launch_knn_scan_packed(a, S_(st));
}

int mgp_knn_scan_bf16x2_d8(const float* train, const void* packed_train, const float* train_sqn, int64_t n, int d,
                           const float* queries, const void* packed_queries, const float* query_sqn,
                           const int64_t* self_idx, int64_t m, int k, int64_t start, float* best_d, int32_t* best_i,
                           int32_t* overflow, void* st) {
  if (n < 0 || m < 0 || d < 1 || k < 1 || start < 0) return MGP_EINVAL;
  if (d > 8) return MGP_EUNSUPPORTED;
  if (m == 0 || start >= n) return MGP_OK;
  if (!train || !packed_train || !train_sqn || !queries || !packed_queries || !query_sqn || !best_d || !best_i ||
      !overflow)
    return MGP_EINVAL;
  KnnPackedArgs a{train, packed_train, train_sqn, queries, packed_queries, query_sqn, self_idx, best_d, best_i,
                  overflow, n, m, start, d, k};
  a.layout = 1;
  return launch_knn_scan_packed(a, S_(st));
}

#define MGP_DEFINE_COEF(SUF, T)                                                                                     \
  int mgp_fast_coefficients_##SUF(const T* fn, int d, const int64_t* ni, int64_t b, int k, const T* tg, int nm,      \
                                  double eps, const T* nd, int kid, int mid, const T* ls, int lsc, T* coeffs,        \
                                  int* info, void* st) {                                                             \
    return fast_coefficients<T>(fn, d, ni, b, k, tg, nm, eps, nd, kid, mid, ls, lsc, coeffs, info, st);              \
  }
MGP_DEFINE_COEF(f32, float)
MGP_DEFINE_COEF(f64, double)

int64_t mgp_fast_coefficients_workspace_bytes(int elem_size, int k, int R, int64_t b) {
  if ((elem_size != 4 && elem_size != 8) || k < 1 || R < 1 || b < 0 || (int64_t)k + 1 + R > kLargeMaxRows) return 0;
  return coefficients_need_workspace(elem_size, k, R) ? large_workspace_bytes(elem_size, k, R, b) : 0;
}
#define MGP_DEFINE_COEF_ANY(SUF, T)                                                                                 \
  int mgp_fast_coefficients_any_##SUF(const T* fn, int d, const int64_t* ni, int64_t b, int k, const T* tg, int R,   \
                                      int nm, double eps, const T* nd, int kid, int mid, const T* ls, int lsc,       \
                                      T* coeffs, int* info, void* workspace, int64_t workspace_bytes, void* st) {    \
    return fast_coefficients_any<T>(fn, d, ni, b, k, tg, R, nm, eps, nd, kid, mid, ls, lsc, coeffs, info, workspace, \
                                    workspace_bytes, st);                                                            \
  }
MGP_DEFINE_COEF_ANY(f32, float)
MGP_DEFINE_COEF_ANY(f64, double)

int64_t mgp_fast_coefficients_gen_workspace_bytes(int elem_size, int k, int R, int64_t b) {
  if ((elem_size != 4 && elem_size != 8) || k < 1 || R < 1 || b < 0 || (int64_t)k + 1 + R > kLargeMaxRows) return 0;
  return coefficients_gen_need_workspace(elem_size, k, R) ? large_workspace_bytes(elem_size, k, R, b) : 0;
}
#define MGP_DEFINE_COEF_GEN(SUF, T)                                                                                 \
  int mgp_fast_coefficients_gen_##SUF(const T* fn, int d, const int64_t* ni, int64_t b, int k, const T* tg, int R,   \
                                      int nm, double eps, const T* nd, double smoothness, int mid, const T* ls,      \
                                      int lsc, T* coeffs, int* info, void* workspace, int64_t workspace_bytes,       \
                                      void* st) {                                                                    \
    return fast_coefficients_gen<T>(fn, d, ni, b, k, tg, R, nm, eps, nd, smoothness, mid, ls, lsc, coeffs, info,     \
                                    workspace, workspace_bytes, st);                                                 \
  }                                                                                                                  \
  int mgp_fast_posterior_mean_gen_##SUF(const T* fq, const T* fn, int d, const int64_t* bi, const int64_t* ni,       \
                                        int64_t b, int k, const T* coeffs, const int64_t* crow, int R,               \
                                        double smoothness, int mid, const T* ls, int lsc, T* mean, void* st) {       \
    return fast_posterior_mean_gen<T>(fq, fn, d, bi, ni, b, k, coeffs, crow, R, smoothness, mid, ls, lsc, mean, st); \
  }
MGP_DEFINE_COEF_GEN(f32, float)
MGP_DEFINE_COEF_GEN(f64, double)

#define MGP_DEFINE_BWD(SUF, T)                                                                                      \
  int mgp_posterior_backward_##SUF(const T* fq, const T* fn, int d, const int64_t* bi, const int64_t* ni, int64_t b, \
                                   int k, const T* tg, int R, int nm, double eps, const T* nd, int kid, int mid,     \
                                   const T* ls, int lsc, const T* gmean, const T* gvar, T* gfq, T* gfn, T* gtg,     \
                                   T* gls, T* gnz, int* info, void* st) {                                            \
    return posterior_backward<T>(fq, fn, d, bi, ni, b, k, tg, R, nm, eps, nd, kid, mid, ls, lsc, gmean, gvar, gfq,  \
                                 gfn, gtg, gls, gnz, info, st);                                                      \
  }                                                                                                                  \
  int mgp_loocv_backward_##SUF(const T* feat, int d, const int64_t* bi, const int64_t* ni, int64_t b, int k,        \
                               const T* tg, int nm, double eps, const T* nd, int kid, int mid, const T* ls, int lsc, \
                               const T* gmean, const T* gvar, const T* gyk, T* gls, T* gnz, int* info, void* st) {   \
    if (b > 0 && (!gmean || !gvar || !gyk || (!gls && !gnz))) return MGP_EINVAL;                                     \
    return posterior_backward<T>(feat, feat, d, bi, ni, b, k, tg, 1, nm, eps, nd, kid, mid, ls, lsc, gmean, gvar,    \
                                 nullptr, nullptr, nullptr, gls, gnz, info, st, gyk);                                \
  }
MGP_DEFINE_BWD(f32, float)
MGP_DEFINE_BWD(f64, double)
int mgp_max_nn_count_backward(int elem_size) { return max_nn_count_backward(elem_size); }
int mgp_max_nn_count_backward_gen(int elem_size) {
  if (elem_size != 4 && elem_size != 8) return MGP_EINVAL;
  return max_nn_count_backward_gen(elem_size);
}
#define MGP_DEFINE_BWD_GEN(SUF, T)                                                                                  \
  int mgp_posterior_backward_gen_##SUF(const T* fq, const T* fn, int d, const int64_t* bi, const int64_t* ni,        \
                                       int64_t b, int k, const T* tg, int R, int nm, double eps, const T* nd,        \
                                       double smoothness, int mid, const T* ls, int lsc, const T* gmean,             \
                                       const T* gvar, const T* gyk, T* gfq, T* gfn, T* gtg, T* gls, T* gnz, T* gnu,  \
                                       int* info, void* st) {                                                        \
    return posterior_backward_gen<T>(fq, fn, d, bi, ni, b, k, tg, R, nm, eps, nd, smoothness, mid, ls, lsc, gmean,   \
                                     gvar, gyk, gfq, gfn, gtg, gls, gnz, gnu, info, st);                             \
  }
MGP_DEFINE_BWD_GEN(f32, float)
MGP_DEFINE_BWD_GEN(f64, double)

int64_t mgp_backward_large_workspace_bytes(int elem_size, int k, int64_t b) {
  if ((elem_size != 4 && elem_size != 8) || k < 1 || b < 0 || (int64_t)k + 2 > kLargeMaxRows) return 0;
  return backward_large_workspace_bytes(elem_size, k, b);
}
#define MGP_DEFINE_BWD_LARGE(SUF, T)                                                                                \
  int mgp_hyper_backward_large_##SUF(const T* feat, int d, const int64_t* bi, const int64_t* ni, int64_t b, int k,   \
                                     const T* tg, int R, int nm, double eps, const T* nd, int kid, int mid,          \
                                     const T* ls, int lsc, const T* gmean, const T* gvar, const T* gyk, T* gls,      \
                                     T* gnz, int* info, void* workspace, int64_t workspace_bytes, void* st) {        \
    return hyper_backward_large<T>(feat, d, bi, ni, b, k, tg, R, nm, eps, nd, kid, mid, ls, lsc, gmean, gvar, gyk,   \
                                   gls, gnz, info, workspace, workspace_bytes, st);                                  \
  }
MGP_DEFINE_BWD_LARGE(f32, float)
MGP_DEFINE_BWD_LARGE(f64, double)
int mgp_backward_gen_large_max_nn_count(int elem_size) {
  if (elem_size != 4 && elem_size != 8) return MGP_EINVAL;
  return backward_gen_large_max_nn_count(elem_size);
}
#define MGP_DEFINE_BWD_GEN_LARGE(SUF, T)                                                                            \
  int mgp_hyper_backward_gen_large_##SUF(const T* feat, int d, const int64_t* bi, const int64_t* ni, int64_t b,      \
                                         int k, const T* tg, int R, int nm, double eps, const T* nd,                 \
                                         double smoothness, int mid, const T* ls, int lsc, const T* gmean,           \
                                         const T* gvar, const T* gyk, T* gls, T* gnz, T* gnu, int* info,             \
                                         void* workspace, int64_t workspace_bytes, void* st) {                       \
    return hyper_backward_gen_large<T>(feat, d, bi, ni, b, k, tg, R, nm, eps, nd, smoothness, mid, ls, lsc, gmean,   \
                                       gvar, gyk, gls, gnz, gnu, info, workspace, workspace_bytes, st);              \
  }
MGP_DEFINE_BWD_GEN_LARGE(f32, float)
MGP_DEFINE_BWD_GEN_LARGE(f64, double)
#define MGP_DEFINE_BWD_LARGE_FULL(SUF, T)                                                                          \
  int mgp_posterior_backward_large_##SUF(const T* fq, const T* fn, int d, const int64_t* bi, const int64_t* ni,      \
                                         int64_t b, int k, const T* tg, int R, int nm, double eps, const T* nd,      \
                                         int kid, int mid, const T* ls, int lsc, const T* gmean, const T* gvar,      \
                                         T* gfq, T* gfn, T* gtg, T* gls, T* gnz, int* info, void* workspace,         \
                                         int64_t workspace_bytes, void* st) {                                        \
    return posterior_backward_large<T>(fq, fn, d, bi, ni, b, k, tg, R, nm, eps, nd, kid, mid, ls, lsc, gmean, gvar,  \
                                       gfq, gfn, gtg, gls, gnz, info, workspace, workspace_bytes, st);               \
  }
MGP_DEFINE_BWD_LARGE_FULL(f32, float)
MGP_DEFINE_BWD_LARGE_FULL(f64, double)

#define MGP_DEFINE(SUF, T)                                                                                           \
  int mgp_crosswise_diffs_##SUF(const T* fq, const T* fn, int d, const int64_t* bi, const int64_t* ni, int64_t b,    \
                                int k, T* out, void* st) {                                                           \
    if (!fq || !fn || !ni || !out || b < 0 || k < 1 || d < 1) return MGP_EINVAL;                                     \
    return launch_crosswise_diffs<T>(fq, fn, d, bi, ni, b, k, out, S_(st));                                          \
  }                                                                                                                  \
  int mgp_pairwise_diffs_##SUF(const T* f, int d, const int64_t* ni, int64_t b, int k, T* out, void* st) {           \
    if (!f || !ni || !out || b < 0 || k < 1 || d < 1) return MGP_EINVAL;                                             \
    return launch_pairwise_diffs<T>(f, d, ni, b, k, out, S_(st));                                                    \
  }                                                                                                                  \
  int mgp_crosswise_dists_##SUF(const T* fq, const T* fn, int d, const int64_t* bi, const int64_t* ni, int64_t b,    \
                                int k, int mid, T* out, void* st) {                                                  \
    if (!fq || !fn || !ni || !out || b < 0 || k < 1 || d < 1 || !valid_metric(mid)) return MGP_EINVAL;               \
    return launch_crosswise_dists<T>(fq, fn, d, bi, ni, b, k, mid, out, S_(st));                                     \
  }                                                                                                                  \
  int mgp_pairwise_dists_##SUF(const T* f, int d, const int64_t* ni, int64_t b, int k, int mid, T* out, void* st) {  \
    if (!f || !ni || !out || b < 0 || k < 1 || d < 1 || !valid_metric(mid)) return MGP_EINVAL;                       \
    return launch_pairwise_dists<T>(f, d, ni, b, k, mid, out, S_(st));                                               \
  }                                                                                                                  \
  int mgp_reduce_diffs_##SUF(const T* diffs, int64_t n, int d, const T* ls, int mid, T* out, void* st) {             \
    if (!diffs || !out || n < 0 || d < 1 || !valid_metric(mid)) return MGP_EINVAL;                                   \
    return launch_reduce_diffs<T>(diffs, n, d, ls, mid, out, S_(st));                                                \
  }                                                                                                                  \
  int mgp_kernel_apply_##SUF(const T* in, int64_t n, int kid, double scale, T* out, void* st) {                      \
    if (!in || !out || n < 0 || !valid_kernel(kid)) return MGP_EINVAL;                                               \
    return launch_kernel_apply<T>(in, n, kid, scale, out, S_(st));                                                   \
  }                                                                                                                  \
  int mgp_matern_gen_##SUF(const T* in, int64_t n, double in_scale, double smoothness, T* out, void* st) {           \
    if (!in || !out || n < 0) return MGP_EINVAL;                                                                     \
    return launch_matern_gen<T>(in, n, in_scale, smoothness, out, S_(st));                                           \
  }                                                                                                                  \
  int mgp_perturb_##SUF(const T* Kin, int64_t b, int k, int nm, double eps, const T* nd, T* out, void* st) {         \
    if (!Kin || !out || b < 0 || k < 1) return MGP_EINVAL;                                                           \
    if (nm != MGP_NOISE_SCALAR && nm != MGP_NOISE_BATCH) return MGP_EINVAL;                                          \
    if (nm == MGP_NOISE_BATCH && !nd) return MGP_EINVAL;                                                             \
    return launch_perturb<T>(Kin, b, k, nm, eps, nd, out, S_(st));                                                   \
  }                                                                                                                  \
  int mgp_solve_##SUF(const T* Kin, const T* Kc, const T* Y, int64_t b, int k, int R, double kout, T* mean, T* var,  \
                      T* yk, T* coeffs, int* info, void* st) {                                                       \
    return solve<T>(Kin, Kc, Y, b, k, R, kout, mean, var, yk, coeffs, info, st);                                     \
  }                                                                                                                  \
  int mgp_loss_sums_##SUF(const T* pred, const T* target, const T* var, int64_t n, const double* scale_dev,          \
                          double hd, double ld, double* out, double* scratch, void* st) {                            \
    if (!pred || !target || !out || n < 0 || !(hd > 0) || !(ld > 0)) return MGP_EINVAL;                              \
    return launch_loss_sums<T>(pred, target, var, n, scale_dev, hd, ld, out, scratch, S_(st));                       \
  }                                                                                                                  \
  int mgp_column_sums_##SUF(const T* x, int64_t n, int R, double* out, double* scratch, void* st) {                  \
    if (!x || !out || n < 0 || R < 0) return MGP_EINVAL;                                                             \
    return launch_column_sums<T>(x, n, R, out, scratch, S_(st));                                                     \
  }

#define MGP_DEFINE_FAST(SUF, T)                                                                                     \
  int mgp_fast_posterior_mean_##SUF(const T* fq, const T* fn, int d, const int64_t* bi, const int64_t* ni, int64_t b, \
                                    int k, const T* coeffs, const int64_t* crow, int R, int kid, int mid,            \
                                    const T* ls, int lsc, T* mean, void* st) {                                       \
    return fast_posterior_mean<T>(fq, fn, d, bi, ni, b, k, coeffs, crow, R, kid, mid, ls, lsc, mean, st);            \
  }
MGP_DEFINE_FAST(f32, float)
MGP_DEFINE_FAST(f64, double)

#define MGP_DEFINE_SHEAR(SUF, T)                                                                                    \
  int mgp_shear_tensor_##SUF(const T* diffs, int64_t G, int n, int m, int variant, double ls, T* out, void* st) {     \
    return shear_tensor<T>(diffs, G, n, m, variant, ls, out, st);                                                    \
  }                                                                                                                  \
  int mgp_solve_multi_##SUF(const T* Kin, const T* Kc, const T* Y, int64_t b, int n, int m, int R, T* mean, T* kk,   \
                            T* yk, int* info, void* st) {                                                            \
    return solve_multi<T>(Kin, Kc, Y, b, n, m, R, mean, kk, yk, info, st);                                           \
  }                                                                                                                  \
  int mgp_shear_posterior_##SUF(const T* fq, const T* fn, const int64_t* bi, const int64_t* ni, int64_t b, int k,    \
                                int in, const T* tg, int64_t ts, int tb, double ls, int nm, double eps, T* mean,     \
                                T* kk, T* yk, int* info, void* st) {                                                 \
    return shear_posterior<T>(fq, fn, bi, ni, b, k, in, tg, ts, tb, ls, nm, eps, mean, kk, yk, info, st);            \
  }
MGP_DEFINE_SHEAR(f32, float)
MGP_DEFINE_SHEAR(f64, double)

#define MGP_DEFINE_CLASS(SUF, T)                                                                                    \
  int mgp_class_sums_##SUF(const T* pred, const void* target, int64_t ts, const int64_t* bi, int64_t b, int R,       \
                           int loss_id, double grad_scale, double hd, T* grad_pred, double* partials,                \
                           double* scratch, void* st) {                                                              \
    if (b < 0 || R < 0 || !(hd > 0)) return MGP_EINVAL;                                                              \
    if (loss_id != MGP_CLASS_LOSS_CROSS_ENTROPY && loss_id != MGP_CLASS_LOSS_MSE) return MGP_EINVAL;                 \
    if (!partials || !scratch || (b > 0 && (!pred || !target))) return MGP_EINVAL;                                   \
    if (ts % (int64_t)sizeof(T) != 0 || (!bi && ts < (int64_t)(R * sizeof(T)))) return MGP_EINVAL;                   \
    return launch_class_sums<T>(pred, target, ts, bi, b, R, loss_id, grad_scale, hd, grad_pred, partials, scratch,   \
                                S_(st));                                                                             \
  }                                                                                                                  \
  int mgp_class_partition_##SUF(const T* labels, int64_t n, int R, const int64_t* ni, int64_t b, int k, T* pred,     \
                                unsigned char* nonconstant, int64_t* count, int64_t* sel, int64_t* nn_sel,           \
                                void* scratch, void* st) {                                                           \
    if (n < 1 || R < 1 || b < 0 || k < 1) return MGP_EINVAL;                                                         \
    if (!labels || !count || !scratch) return MGP_EINVAL;                                                            \
    if (b > 0 && (!ni || !pred || !nonconstant || !sel || !nn_sel)) return MGP_EINVAL;                               \
    return launch_class_partition<T>(labels, n, R, ni, b, k, pred, nonconstant, count, sel, nn_sel, scratch, S_(st)); \
  }                                                                                                                  \
  int mgp_class_scatter_##SUF(const T* src_mean, const T* src_var, const int64_t* sel, int64_t m, int64_t b, int R,  \
                              T* dst_mean, T* dst_var, void* st) {                                                   \
    if (m < 0 || b < 0 || m > b || R < 1) return MGP_EINVAL;                                                         \
    if (m > 0 && (!src_mean || !sel || !dst_mean || ((src_var != nullptr) != (dst_var != nullptr))))                 \
      return MGP_EINVAL;                                                                                             \
    return launch_class_scatter<T>(src_mean, src_var, sel, m, b, R, dst_mean, dst_var, S_(st));                      \
  }
MGP_DEFINE_CLASS(f32, float)
MGP_DEFINE_CLASS(f64, double)

MGP_DEFINE(f32, float)
MGP_DEFINE(f64, double)

}  // extern "C"
