// Host side of the register-resident wave kernel family (fused_wave_kernel: forward, dealt-triangle backward, row-per-lane
// backward; built in or compiled at run time): the ONE place that knows how many bytes of dynamic LDS the kernel's layout
// takes and what goes into WaveGeom (wave_geometry), the persistent grid (wave_grid), and everything from the occupancy
// lookup to the noted kernel name (wave_launch).  Included by the translation units that instantiate launch_np_impl
// (mgp_fused_wave_inst_*.hip: the instantiations of mgp_fused_wave_list.h), by the dispatcher (mgp_fused_wave.hip) and
// by the backward launchers (mgp_backward_dlt.hip).
#pragma once
#include <cmath>

#include "mgp_fused_wave_kernel.h"
#include "mgp_gen_launch.h"

namespace mgp {

#ifdef MGP_DEBUG_HOOKS
extern int g_phase_mask;
extern int g_grid_per_cu;  // override of resident workgroups per CU
extern int g_lds_pad;      // extra dynamic LDS bytes per workgroup
#endif

// One instantiation: the kernel's template arguments as values (static k / R / d, or 0), and whether it was compiled at
// run time (mgp_jit.hip) or is built into the library.
struct WaveShape {
  int es, NP, kfix, rfix, dfix;
  bool piped, coeff, packed, gram, gen64, bwd, jit;
};
constexpr WaveDims wave_dims(const WaveShape& s) { return wave_dims(s.es, s.NP, s.kfix, s.rfix, s.dfix, s.coeff, s.gram); }

// Shapes built into the library: forward, mgp_fused_wave_list.h (BASELINE configs 2/3 and 4, one response); backward,
// mgp_backward_dlt.hip (config 4 in fp64 on the dealt triangle, config 3 in fp32 in the Gram form).
inline bool wave_builtin(int es, int k, int R, int d, bool gram, bool gen64, bool bwd) {
  if (bwd) return es == 8 ? (k == 50 && d == 8) : (k == 30 && d == 40 && gram);
  return !gen64 && R == 1 && ((k == 30 && d == 40) || (k == 50 && d == 8));
}

// fp32 pipelined kernels compute the squared distances in the Gram form, except for the Matern-1/2
// kernel (and the general Matern below nu = 1): exp(-r) has a kink at r = 0, so the absolute error a
// cancelling Gram form leaves in a tiny squared distance (duplicated training points) would show up at
// first order there.
// In fp64 the Gram form (MGP_GRAM64) would serve every kernel but the general Matern, which has instantiations of its
// own: its absolute error in a squared distance, ~1e-16 r^2, is eleven orders below the 1e-5 the results are held to.
// The backward is in the difference form in fp64.  (A caller without a smoothness -- the prepare_* functions -- passes 1.)
inline bool wave_gram(int es, int kernel_id, double smoothness, bool bwd = false) {
  if (!MGP_GRAM) return false;
  if (es == 8) return !bwd && MGP_GRAM64 != 0 && kernel_id != MGP_KERNEL_MATERN_GEN;
  return kernel_id != MGP_KERNEL_MATERN_05 && !(kernel_id == MGP_KERNEL_MATERN_GEN && smoothness < 1.0);
}

// every address and stride a 16-byte gather depends on, or-ed together
inline uintptr_t wave_align(const FusedArgs& a, bool packed) {
  return packed ? ((uintptr_t)a.packed_q | (uintptr_t)a.packed_nn | (uintptr_t)a.q_stride | (uintptr_t)a.nn_stride)
                : ((uintptr_t)a.feat_q | (uintptr_t)a.feat_nn);
}

struct WaveLaunch {
  WaveGeom g;
  size_t lds;  // dynamic LDS bytes per workgroup
  int nh;      // neighbourhoods per task
  int status;  // MGP_OK, or why this instantiation cannot serve the call
};

// The kernel's LDS layout (mgp_fused_wave_kernel.h: tile, exchange images, column buffers / row addresses, node table)
// in bytes, and its WaveGeom.  (g.q is read by the run-time-shape instantiations only.)
inline WaveLaunch wave_geometry(const FusedArgs& a, const WaveShape& s) {
  const WaveDims WD = wave_dims(s);
  const size_t es = (size_t)s.es;
  const bool row_bwd = s.bwd && !WD.DLT;
  WaveLaunch w{};
  WaveGeom& g = w.g;
  w.nh = WD.NH;
  g.mask = 0xF;
  g.q = s.NP - 1 - a.R;
  const int dpad = (a.d + WD.CH - 1) / WD.CH * WD.CH, dcap = row_bwd && s.es == 4 ? 128 : 64;  // (fp32 row-per-lane backward: rows of up to 128 features in one stage)
  g.dst = dpad < dcap ? dpad : dcap;
  g.xs = g.dst + WD.E;  // dst/E is even -> dst/E + 1 slots: odd
  g.vec_ok = (a.d % WD.E == 0) && (wave_align(a, s.packed) % 16 == 0);
  g.ntasks = (a.b + WD.NH - 1) / WD.NH;
  w.status = MGP_EUNSUPPORTED;
  if (s.packed && a.R > WD.E && !a.targets_batch) return w;  // the responses ride in one 16-byte slot
  if ((s.dfix > 0 || s.piped) && !g.vec_ok) return w;
  if (s.piped && a.d > g.dst) return w;  // more than one feature stage
  // (the general Matern needs the per-lane pair tables: 32-slot or static shapes; fp64 -- round 4 -- in the GEN64
  // instantiations only)
  const bool gen = a.kernel_id == MGP_KERNEL_MATERN_GEN;
  if (gen ? !((s.NP <= 32 || s.kfix > 0) && !s.coeff && (s.es == 4 || s.gen64)) : s.gen64) return w;
  w.status = MGP_OK;

  const size_t tile_feat = (size_t)wave_tile_rows(WD, s.NP, s.kfix, g.xs) * g.xs + wave_stage_elems(WD);
  size_t lds;
  if (s.bwd) {
    // the image lies BEHIND the tile; row per lane: whole rows (the packed triangle of the 64-slot forward does not
    // apply), and behind both the column buffers / norm array / row addresses or the two solved vectors of both
    // neighbourhoods (128 entries) -- unless everything that lived there has another home (wave_bwd_tailfree)
    const size_t kmat = row_bwd ? (size_t)s.NP * (s.NP + WD.E) : (size_t)WD.KMAT, vecs = 128 * es;
    size_t tail = wave_colbuf_bytes(s.es, s.NP, false);
    if (row_bwd) tail = wave_bwd_tailfree(s.es, s.NP, s.gram, g.dst) ? 0 : (tail > vecs ? tail : vecs);
    lds = (tile_feat + (size_t)WD.NH * kmat) * es + tail;
  } else {
    const size_t tile_mat = (size_t)WD.NH * WD.KMAT, tile_elems = tile_feat > tile_mat ? tile_feat : tile_mat;
    lds = s.piped ? tile_elems * es + wave_colbuf_bytes(s.es, s.NP, wave_fold(s.es, s.NP, s.kfix, s.rfix, s.dfix, s.piped, s.coeff, s.gram))
                  : (tile_elems + 64 + g.dst + (g.dst & 1)) * es + 64 * sizeof(int64_t);
  }
  lds = (lds + 15) & ~(size_t)15;
  // general-smoothness Matern: the node table (2 x MGP_GEN_NODES floats) goes behind everything else in LDS; spacing and
  // the log2 of h 2^(1-nu)/Gamma(nu) are launch constants.  (The backward serves no such kernel and reserves nothing.)
  // (the constants and the table's size: gen_launch_constants / gen_table_bytes, shared with the workgroup families)
  g.gen_h = 0.5f;
  g.gen_h64 = 0.3;
  g.gen_xmin64 = 1e-12;
  if (gen) {
    const GenLaunch c = gen_launch_constants(a.smoothness, s.es == 8);
    g.gen_tab = s.bwd ? 0 : (int)lds;
    g.gen_h = c.h;
    g.gen_lc = c.lc;
    if (s.es == 8) g.gen_h64 = c.h64, g.gen_lc64 = c.lc64, g.gen_xmin64 = c.xmin64;
    if (!s.bwd) lds += gen_table_bytes(s.es);
  }
#ifdef MGP_DEBUG_HOOKS
  if (!s.bwd && !s.jit) g.mask = g_phase_mask, lds += (size_t)g_lds_pad;
#endif
  w.lds = lds;
  return w;
}

// Occupancy experiments: the environment may lower the resident workgroups per CU, one variable per launcher.
enum { kEnvWavePerCu, kEnvJitPerCu, kEnvBwdDltPerCu, kEnvBwdRowPerCu, kEnvNoPerCu };
inline int wave_env(const WaveShape& s) {
  if (!s.bwd) return s.jit ? kEnvJitPerCu : kEnvWavePerCu;
  if (!wave_dims(s).DLT) return kEnvBwdRowPerCu;
  return s.jit ? kEnvNoPerCu : kEnvBwdDltPerCu;
}

// Persistent grid = exactly the resident capacity: every workgroup owns a fixed share of the
// tasks, so one workgroup more than fits runs as a second, nearly empty round (measured: 13
// instead of 12 per CU costs 40 %).  Whole eights, at least one, no more than the tasks need.
inline int wave_grid(int es, int NP, int kfix, bool bwd, int env, bool tree, int cus, int per_cu, int64_t ntasks, int64_t* out) {
#ifdef MGP_DEBUG_HOOKS
  if (!bwd && g_grid_per_cu > 0) per_cu = g_grid_per_cu;
#endif
  // (fp64, 32 slots, run-time shape: two waves per SIMD although three would fit -- measured, mgp_fused_wave_kernel.h)
  if (es == 8 && NP == 32 && kfix == 0 && per_cu > 8) per_cu = 8;
  static const int env_per_cu[] = {env_int("MGP_WAVE_PER_CU"), env_int("MGP_JIT_PER_CU"), env_int("MGP_BWD_DLT_PER_CU"),
                                   env_int("MGP_BWD_ROW_PER_CU"), 0};
  if (env_per_cu[env] > 0 && env_per_cu[env] < per_cu) per_cu = env_per_cu[env];
  int64_t grid = (int64_t)cus * per_cu / 8 * 8;
  if (grid < 8) grid = 8;
  if (grid > ntasks) grid = (ntasks + 7) / 8 * 8;
  // (one-launch LOOCV evaluation: the leaves of the reduction tree are this launch's workgroups)
  if (tree && grid > kTreeMaxLeaves) return MGP_EUNSUPPORTED;
  *out = grid;
  return MGP_OK;
}

// From the residency of this kernel at this LDS size (the occupancy query; the CU count from the device) to the launch
// and what the library remembers of it.  Kernel: `const void*` (built in) or hipFunction_t (compiled at run time).
template <typename Kernel>
int wave_launch(Kernel fn, Residency& res, const FusedArgs& a, const WaveShape& s, WaveLaunch& w, hipStream_t stream) {
  int per_cu = 0, cus = 0;
  const int rrc = res.lookup(fn, 64, w.lds, &per_cu, &cus);
  if (rrc != MGP_OK) return rrc;
  int64_t grid = 0;
  const int grc = wave_grid(s.es, s.NP, s.kfix, s.bwd, wave_env(s), a.tree.out != nullptr, cus, per_cu, w.g.ntasks, &grid);
  if (grc != MGP_OK) return grc;
  FusedArgs al = a;
  al.tree.grid = (int)grid;  // (the leaves of the reduction tree are this launch's workgroups)
  al.tree.nh = w.nh;
  if (a.tree.mode == kTreeThreeLaunch) al.tree.out = nullptr;  // (the caller walks these leaves by kernels behind the launch)
  auto tf = [](bool v) { return v ? "true" : "false"; };
  const LaunchLabel label(a.b, a.k, a.d, a.R, "mgp::fused_wave_kernel<%s,%d,%d,%d,%d,%s,%s,%s,%s%s>%s", s.es == 4 ? "float" : "double", s.NP,
                          s.kfix, s.rfix, s.dfix, tf(s.piped), tf(s.coeff), tf(s.packed), tf(s.gram),
                          s.bwd ? ",false,backward" : (s.gen64 ? ",gen64" : ""), s.jit ? " [run-time compiled]" : "");
  void* params[] = {&al, &w.g};
  const int lrc = launch_noted(fn, grid, 64, w.lds, per_cu, stream, params, &label);  // (which instantiation served a call)
  if (lrc != MGP_OK) return lrc;
  if (!s.bwd) note_tree_geometry(a.tree.out ? (int)grid : 0, w.nh);
  return MGP_OK;
}

template <typename T, int NP, int KFIX, int RFIX, int DFIX, bool PIPED, bool COEFF, bool PACKED, bool GRAM, bool GEN64>
int launch_np_impl(const FusedArgs& a, hipStream_t stream) {
  if (COEFF && a.tree.out) return MGP_EINVAL;
  constexpr WaveShape S{(int)sizeof(T), NP, KFIX, RFIX, DFIX, PIPED, COEFF, PACKED, GRAM, GEN64, false, false};
  WaveLaunch w = wave_geometry(a, S);
  if (w.status != MGP_OK) return w.status;
  static Residency res;
  return wave_launch(reinterpret_cast<const void*>(&fused_wave_kernel<T, NP, KFIX, RFIX, DFIX, PIPED, COEFF, PACKED, GRAM, GEN64>), res, a,
                     S, w, stream);
}

}  // namespace mgp
