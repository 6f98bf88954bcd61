// Host side of every launcher outside the k-NN scans: the ONE place that knows the LDS of a CU and its allocation
// granule, the grid of a persistent kernel, the feature chunk that fits, and the tail of a launch -- from the grid to
// the kernel name and geometry the library remembers (mgp_last_kernel_name, mgp_last_launch_geometry).  A launcher keeps
// what belongs to its kernel's layout: its LDS byte formula, thread count, geometry struct, refusals and variants.
// Host only: a run-time compile of the kernels (mgp_jit.hip) never sees this file.
#pragma once
#ifndef __HIPCC_RTC__

#include <climits>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>

#include "mgp_args.h"

namespace mgp {

// ---- constants and pure rules ------------------------------------------------------------------------------------------
constexpr size_t kCuLdsBytes = 160 * 1024;  // the LDS of a CU (gfx950): the most one workgroup can ask for
// measured on gfx950: LDS is handed out in granules of this many bytes (13 x 12192 B is refused, 12 x 12704 B fits)
constexpr size_t kLdsGranule = 1280;
constexpr size_t kLdsOptIn = 64 * 1024;  // dynamic LDS beyond this is the kernel's only after allow_dynamic_lds
// the CUs the capacity grids assume (MI300X / MI355X; a device with fewer runs the surplus as a second round)
constexpr int64_t kAssumedCus = 256LL;

// workgroups of `lds_bytes` each that fit the LDS of a CU (0 where one does not fit; no LDS: no bound)
inline int lds_workgroups_per_cu(size_t lds_bytes) {
  if (lds_bytes == 0) return INT_MAX;
  return (int)(kCuLdsBytes / ((lds_bytes + kLdsGranule - 1) / kLdsGranule * kLdsGranule));
}

// Persistent grid = the resident capacity of the assumed device (the kernels grid-stride over the rest): one workgroup
// more than fits would run as a second, nearly empty round (measured on the wave kernels: 13 instead of 12 per CU costs
// 40 %).  At least one and at most `max_per_cu` workgroups per CU, no more than the work units, nor than the slabs of a
// workspace that gives every workgroup one.
inline int capacity_per_cu(size_t lds_bytes, int max_per_cu) {
  const int per_cu = lds_workgroups_per_cu(lds_bytes);
  return per_cu < 1 ? 1 : (per_cu > max_per_cu ? max_per_cu : per_cu);
}
struct Capacity {
  int max_per_cu;
  int64_t slabs = INT64_MAX;
};
inline int64_t capacity_grid(int64_t units, size_t lds_bytes, Capacity cap) {
  int64_t g = kAssumedCus * capacity_per_cu(lds_bytes, cap.max_per_cu);
  if (g > cap.slabs) g = cap.slabs;
  return units < g ? units : g;
}

// Feature chunk of a workgroup kernel that stages rows in LDS: a multiple of 8 (whole 16-byte pieces, odd slot count with
// the pad), as wide as fits next to whatever else `lds_bytes(dc)` counts, at most 64, at least 8.
struct FeatureChunk {
  int dc;
  size_t lds;
  bool fits;  // false: not even 8 features fit
};
template <typename LdsBytes>
FeatureChunk feature_chunk(int d, LdsBytes&& lds_bytes) {
  int dc = d < 64 ? (d + 7) / 8 * 8 : 64;
  while (dc > 8 && lds_bytes(dc) > kCuLdsBytes) dc -= 8;
  const size_t lds = lds_bytes(dc);
  return {dc, lds, lds <= kCuLdsBytes};
}

// the largest k >= 1 up to which fits(k) holds without a gap (the mgp_*max_nn_count limits; fits(1) is taken as given)
template <typename Fits>
int largest_k(Fits&& fits) {
  int k = 1;
  while (fits(k + 1)) ++k;
  return k;
}

// a kernel gets more than 64 KiB of dynamic LDS only after saying so
template <typename K>
int allow_dynamic_lds(K kernel, size_t lds_bytes) {
  if (lds_bytes <= kLdsOptIn) return MGP_OK;
  const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (int)lds_bytes);
  return e == hipSuccess ? MGP_OK : -(1000 + (int)e);
}

inline int env_int(const char* name) { return getenv(name) ? atoi(getenv(name)) : 0; }
// MGP_TRACE=1: every noted launch (and the run-time compiler) says on stderr what it does
inline bool trace_enabled() {
  static const bool on = getenv("MGP_TRACE") != nullptr;
  return on;
}

// ---- launch tails ----------------------------------------------------------------------------------------------------------
// What MGP_TRACE prints of a launch and the library remembers of it: the kernel's name and the call's shape (-1: the
// launcher has no such number).  A launcher that passes none stays silent: mgp_last_kernel_name keeps the launch before.
struct LaunchLabel {
  char name[160];
  int64_t b;
  int k, d, R;
  LaunchLabel(int64_t b_, int k_, int d_, int R_, const char* fmt, ...) __attribute__((format(printf, 6, 7))) : b(b_), k(k_), d(d_), R(R_) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(name, sizeof(name), fmt, ap);
    va_end(ap);
  }
};

struct Launched {
  int status;
  int64_t grid;
  int per_cu;
};

inline hipError_t launch_on(const void* fn, int64_t grid, int threads, size_t lds, hipStream_t stream, void** params) {
  (void)hipLaunchKernel(fn, dim3((unsigned)grid), dim3((unsigned)threads), params, lds, stream);
  return hipGetLastError();
}
// (a kernel of a run-time compiled module)
inline hipError_t launch_on(hipFunction_t fn, int64_t grid, int threads, size_t lds, hipStream_t stream, void** params) {
  return hipModuleLaunchKernel(fn, (unsigned)grid, 1, 1, (unsigned)threads, 1, 1, (unsigned)lds, stream, params, nullptr);
}

// trace, launch, check, note: the end of every tail.  Kernel: `const void*` (built in) or hipFunction_t.
template <typename Kernel>
int launch_noted(Kernel fn, int64_t grid, int threads, size_t lds, int per_cu, hipStream_t stream, void** params,
                 const LaunchLabel* label) {
  if (label && trace_enabled()) {
    char shape[96] = "";
    int n = 0;
    if (label->b >= 0) n += snprintf(shape + n, sizeof(shape) - n, " b=%lld", (long long)label->b);
    if (label->k >= 0) n += snprintf(shape + n, sizeof(shape) - n, " k=%d", label->k);
    if (label->d >= 0) n += snprintf(shape + n, sizeof(shape) - n, " d=%d", label->d);
    if (label->R >= 0) n += snprintf(shape + n, sizeof(shape) - n, " R=%d", label->R);
    fprintf(stderr, "[mgp] %s%s grid=%lld lds=%zu per_cu=%d\n", label->name, shape, (long long)grid, lds, per_cu);
  }
  const hipError_t err = launch_on(fn, grid, threads, lds, stream, params);
  if (err != hipSuccess) return -(1000 + (int)err);
  if (label) {
    note_launch("%s", label->name);
    note_launch_geometry(grid, lds);
  }
  return MGP_OK;
}

// Residency tail: from the residency of `kernel` at this thread count and LDS size (the occupancy query capped by the LDS
// granule rule, the CU count from the device: Residency, mgp_wave_common.h) to the noted geometry.  Grid = exactly the
// resident capacity, no more than the work units.  per_cu_env: an environment variable that may lower the workgroups
// per CU (occupancy experiments; looked up at every launch that names one), or nullptr.  The arguments are converted to
// the kernel's parameter types.
template <typename Res, typename... P, typename... A>
Launched launch_resident(void (*kernel)(P...), Res& res, int threads, size_t lds, int64_t units, const char* per_cu_env,
                         hipStream_t stream, const LaunchLabel* label, const A&... args) {
  const void* fn = reinterpret_cast<const void*>(kernel);
  int per_cu = 0, cus = 0;
  const int rc = res.lookup(fn, threads, lds, &per_cu, &cus);
  if (rc != MGP_OK) return {rc, 0, 0};
  const int env_per_cu = per_cu_env ? env_int(per_cu_env) : 0;
  if (env_per_cu > 0 && env_per_cu < per_cu) per_cu = env_per_cu;
  int64_t grid = (int64_t)cus * per_cu;
  if (grid > units) grid = units;
  const int status = [&](P... v) {
    void* params[] = {(void*)&v...};
    return launch_noted(fn, grid, threads, lds, per_cu, stream, params, label);
  }(args...);
  return {status, grid, per_cu};
}

// Capacity tail: the same behind a capacity grid (capacity_grid: no query of the device), with the opt-in above 64 KiB.
template <typename... P, typename... A>
Launched launch_capacity(void (*kernel)(P...), int threads, size_t lds, int64_t units, Capacity cap, hipStream_t stream,
                         const LaunchLabel* label, const A&... args) {
  const int rc = allow_dynamic_lds(kernel, lds);
  if (rc != MGP_OK) return {rc, 0, 0};
  const int64_t grid = capacity_grid(units, lds, cap);
  const int per_cu = capacity_per_cu(lds, cap.max_per_cu);
  const int status = [&](P... v) {
    void* params[] = {(void*)&v...};
    return launch_noted(reinterpret_cast<const void*>(kernel), grid, threads, lds, per_cu, stream, params, label);
  }(args...);
  return {status, grid, per_cu};
}

}  // namespace mgp

#endif  // !__HIPCC_RTC__
