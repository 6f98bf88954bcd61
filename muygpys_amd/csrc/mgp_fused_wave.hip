// Host side of the register-resident wave kernels: launch geometry, the precompiled instantiations,
// dispatch.  The kernel itself lives in mgp_fused_wave_kernel.h.
#include <cstdio>
#include <cstdlib>

#include "mgp_fused_wave_launch.h"

namespace mgp {

#ifdef MGP_DEBUG_HOOKS
int g_phase_mask = 0xF;
int g_grid_per_cu = 0;  // override of resident workgroups per CU
int g_lds_pad = 0;      // extra dynamic LDS bytes per workgroup
#endif

// (launch_np_impl is instantiated in mgp_fused_wave_inst_*.hip; here only the calls)
template <typename T, int NP, int KFIX, int RFIX, int DFIX, bool PIPED, bool COEFF, bool PACKED, bool GRAM, bool GEN64 = false>
static int launch_inst(const FusedArgs& a, hipStream_t stream) {
  return launch_np_impl<T, NP, KFIX, RFIX, DFIX, PIPED, COEFF, PACKED, GRAM, GEN64>(a, stream);
}

template <typename T, int NP, int KFIX, int RFIX, int DFIX, bool PIPED, bool COEFF = false, bool PACKED = false>
static int launch_np(const FusedArgs& a, hipStream_t stream) {
  // fp64 general-smoothness Matern: its own instantiations, for the run-time-shape 32-slot kernels (static shapes:
  // compiled at run time, launch_jit); the difference form throughout
  if constexpr (sizeof(T) == 8) {
    if (a.kernel_id == MGP_KERNEL_MATERN_GEN) {
      if constexpr (NP == 32 && KFIX == 0 && !COEFF) return launch_inst<T, NP, KFIX, RFIX, DFIX, PIPED, COEFF, PACKED, false, true>(a, stream);
      else return MGP_EUNSUPPORTED;
    }
  }
  if constexpr (PIPED && !COEFF && MGP_GRAM && (sizeof(T) == 4 || MGP_GRAM64)) {
    if (wave_gram(sizeof(T), a.kernel_id, a.smoothness)) return launch_inst<T, NP, KFIX, RFIX, DFIX, PIPED, COEFF, PACKED, true>(a, stream);
  }
  return launch_inst<T, NP, KFIX, RFIX, DFIX, PIPED, COEFF, PACKED, false>(a, stream);
}

// Slots per neighbourhood of the static instantiation that serves a shape (0: none does): 16 / 32 / 64,
// pipelined gather (16-byte aligned rows, one feature stage), at most four responses in a prepared table.
static int static_slots(int es, int d, int k, int R, bool packed, bool gathered) {
  const int E = 16 / es, CH = 2 * E, rows = k + 1 + R;
  if (k < 1 || R < 1 || rows > 64 || d % E != 0 || (d + CH - 1) / CH * CH > 64) return 0;
  if (packed && !gathered && R > E) return 0;
  return rows <= 16 ? 16 : (rows <= 32 ? 32 : 64);
}

// A static shape the library was not built with: the instantiation compiled at run time (mgp_jit.hip).
// Same geometry code as launch_np_impl, from the shape as run-time values.
template <typename T>
static int launch_jit(const FusedArgs& a, hipStream_t stream) {
  const bool packed = a.packed_nn != nullptr;
  const int NP = static_slots(sizeof(T), a.d, a.k, a.R, packed, a.targets_batch != 0);
  if (NP == 0 || a.coeffs != nullptr) return MGP_EUNSUPPORTED;
  const bool gen64 = sizeof(T) == 8 && a.kernel_id == MGP_KERNEL_MATERN_GEN;
  const WaveShape s{(int)sizeof(T), NP, a.k, a.R, a.d, true, false, packed, wave_gram(sizeof(T), a.kernel_id, a.smoothness), gen64, false, true};
  WaveLaunch w = wave_geometry(a, s);
  if (w.status != MGP_OK) return w.status;  // (unaligned rows: everything else static_slots has refused)
  hipFunction_t fn = nullptr;
  const int jrc = jit_wave_function(s.es, NP, a.k, a.R, a.d, packed, s.gram, &fn, jit_mode() == 2 || a.b >= jit_min_batch(), gen64);
  if (jrc != MGP_OK) return jrc;
  static Residency res;
  return wave_launch(fn, res, a, s, w, stream);
}

template <typename T>
int launch_fused_wave(const FusedArgs& a, hipStream_t stream) {
  const int rows = a.k + 1 + a.R;
  if (a.b >= (int64_t)1 << 31) return MGP_EUNSUPPORTED;  // (task and chunk numbers are 32-bit in the kernel)
  if (a.tree.out && (a.R != 1 || a.coeffs || !a.ykinvy || !a.tree.ctrl || !a.tree.resp)) return MGP_EINVAL;
  if (a.coeffs != nullptr) {  // fused fast-mean precompute: one response
    if (a.packed_nn != nullptr) return MGP_EUNSUPPORTED;
    if (a.R == 1 && rows <= 32) return launch_np<T, 32, 0, 0, 0, false, true>(a, stream);
    if (a.R == 1 && rows <= 64) return launch_np<T, 64, 0, 0, 0, false, true>(a, stream);
    return MGP_EUNSUPPORTED;
  }
  // other static shapes: the instantiation compiled at run time, when allowed and worth it (mgp_jit.hip)
  const bool gen64 = sizeof(T) == 8 && a.kernel_id == MGP_KERNEL_MATERN_GEN;  // (no built-in static instantiation)
  const bool builtin = wave_builtin(sizeof(T), a.k, a.R, a.d, false, gen64, false);
  // (calls from MUYGPYS_HIP_JIT_MIN_BATCH neighbourhoods on may compile; shorter ones, from
  // MUYGPYS_HIP_JIT_CACHED_MIN_BATCH on, take a kernel that is loaded or in the disk cache already)
  const bool try_jit = !builtin && jit_mode() != 0 && (jit_mode() == 2 || a.b >= jit_cached_min_batch());
  if (a.packed_nn != nullptr) {  // prepared tables: the pipelined kernels only
    if (builtin && a.k == 30) return launch_np<T, 32, 30, 1, 40, true, false, true>(a, stream);
    if (builtin && a.k == 50) return launch_np<T, 64, 50, 1, 8, true, false, true>(a, stream);
    if (try_jit) {
      const int rc = launch_jit<T>(a, stream);
      if (rc != MGP_EUNSUPPORTED) return rc;
    }
    if (rows <= 32) return launch_np<T, 32, 0, 0, 0, true, false, true>(a, stream);
    if (rows <= 64) return launch_np<T, 64, 0, 0, 0, true, false, true>(a, stream);
    return MGP_EUNSUPPORTED;
  }
  if (builtin && a.k == 30) {  // BASELINE configs 2/3 (and their fp64 form), all shapes static
    const int rc = launch_np<T, 32, 30, 1, 40, true>(a, stream);
    if (rc != MGP_EUNSUPPORTED) return rc;
  }
  if (builtin && a.k == 50) {  // BASELINE config 4 shape, all shapes static
    const int rc = launch_np<T, 64, 50, 1, 8, true>(a, stream);
    if (rc != MGP_EUNSUPPORTED) return rc;
  }
  if (try_jit) {
    const int rc = launch_jit<T>(a, stream);
    if (rc != MGP_EUNSUPPORTED) return rc;
  }
  // run-time shapes: the pipelined direct-to-LDS gather when the rows allow it (16-byte aligned,
  // d a multiple of 16 bytes, one feature stage), the register-staged gather otherwise
  if (rows <= 32) {
    const int rc = launch_np<T, 32, 0, 0, 0, true>(a, stream);
    return rc != MGP_EUNSUPPORTED ? rc : launch_np<T, 32, 0, 0, 0, false>(a, stream);
  }
  if (rows <= 64) {
    const int rc = launch_np<T, 64, 0, 0, 0, true>(a, stream);
    return rc != MGP_EUNSUPPORTED ? rc : launch_np<T, 64, 0, 0, 0, false>(a, stream);
  }
  return MGP_EUNSUPPORTED;
}

// The instantiation launch_fused_wave would pick for a shape (pure function of its arguments;
// mirrors the dispatch above for 16-byte aligned tables).  Empty string: not a wave-kernel shape.
int describe_fused_wave(int elem_size, int d, int k, int R, int packed, char* buf, int len) {
  const int rows = k + 1 + R, E = 16 / elem_size;
  const char* t = elem_size == 4 ? "float" : "double";
  const bool vec = d % E == 0, one_stage = ((d + 2 * E - 1) / (2 * E)) * (2 * E) <= 64;
  int np = rows <= 32 ? 32 : (rows <= 64 ? 64 : 0), kf = 0, rf = 0, df = 0;
  bool piped = vec && one_stage;
  if (k == 30 && R == 1 && d == 40) kf = 30, rf = 1, df = 40, np = 32, piped = true;
  else if (k == 50 && R == 1 && d == 8) kf = 50, rf = 1, df = 8, np = 64, piped = true;
  else if (jit_mode() != 0 && static_slots(elem_size, d, k, R, packed != 0, false) != 0)  // (large batches: run-time compiled)
    kf = k, rf = R, df = d, np = static_slots(elem_size, d, k, R, packed != 0, false), piped = true;
  if (np == 0 || (packed && (!piped || R > E))) return snprintf(buf, len, "%s", "");
  // (the Gram-form instantiation serves fp32 pipelined shapes for every kernel except Matern-1/2)
  const bool gram = piped && MGP_GRAM && (elem_size == 4 || MGP_GRAM64);
  return snprintf(buf, len, "mgp::fused_wave_kernel<%s,%d,%d,%d,%d,%s,false,%s,%s>", t, np, kf, rf, df,
                  piped ? "true" : "false", packed ? "true" : "false", gram ? "true" : "false");
}

// compile the static instantiation of a shape into the disk cache (no GPU needed)
int prepare_fused_wave(int elem_size, int d, int k, int R, int packed, int kernel_id) {
  const bool gen64 = elem_size == 8 && kernel_id == MGP_KERNEL_MATERN_GEN;  // (fp64 general Matern: an instantiation of its own)
  if (wave_builtin(elem_size, k, R, d, false, gen64, false)) return MGP_OK;
  const int np = static_slots(elem_size, d, k, R, packed != 0, false);
  if (np == 0) return MGP_EUNSUPPORTED;
  return jit_wave_prepare(elem_size, np, k, R, d, packed != 0, wave_gram(elem_size, kernel_id, 1.0), gen64);
}

template int launch_fused_wave<float>(const FusedArgs&, hipStream_t);
template int launch_fused_wave<double>(const FusedArgs&, hipStream_t);

}  // namespace mgp

#if MGP_WAVE_TIMING
extern "C" int mgp_debug_wave_timing(unsigned long long* out, int reset) {
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(mgp::g_wave_timing), sizeof(mgp::g_wave_timing)) != hipSuccess) return -1;
  if (reset) {
    unsigned long long z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (hipMemcpyToSymbol(HIP_SYMBOL(mgp::g_wave_timing), z, sizeof(z)) != hipSuccess) return -1;
  }
  return 0;
}
#endif
