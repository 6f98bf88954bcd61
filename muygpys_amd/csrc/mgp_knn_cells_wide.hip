// Approximate k-NN over an inverted-cell (IVF) index for k-best lists WIDER THAN A WAVE: the per-query scan of the
// probed cells at 1 <= k <= 1024 (mgp_knn_cells.hip stops at 64, the width of its register-held list).
//
// One wave serves one query; the four waves of a workgroup are independent (no barrier, no shared state, no workgroup
// waits on another, no atomics).
//
//   scan    cells_scan_body (mgp_knn_cells_scan.h), the one mgp_knn_cells.hip runs: at equal k both kernels return the
//           same bits.
//   list    mgp_knn_list_wide.h: (distance, position) pairs in LDS, one contiguous run per wave of up to
//           wide_list_slots(k) entries.  The slot count is a run-time value and the LDS is sized at launch, so the
//           kernel is instantiated per row width only (16 times).  At k = 1024 a wave holds 1536 slots = 12 KiB, a
//           workgroup 48 KiB (+ 1 KiB of query rows past d = 32): three workgroups per CU.
//
// Reference: the approximate branch of the reference's neighbour search (hnswlib behind NN_Wrapper,
// src/MuyGPyS/neighbors.py:109-127,213-262), which takes any nn_count; the inverted-cell index fills the same role on a
// GPU.
#include <cstdint>

#include "mgp_args.h"
#include "mgp_knn_cells_scan.h"
#include "mgp_knn_list_wide.h"

namespace mgp {

namespace {

struct CellWideArgs : CellScanArgs {
  int cap;  // wide_list_slots(k)
};

// D4 = d / 4
template <int D4>
__global__ __launch_bounds__(kCellWaves * 64) void knn_cells_wide_kernel(const CellWideArgs a) {
  extern __shared__ float4 s_slots[];  // per wave: cap distances, then cap positions
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t q = (int64_t)blockIdx.x * kCellWaves + wave;
  if (q >= a.m) return;
  float* slots = reinterpret_cast<float*>(s_slots) + (size_t)wave * 2 * a.cap;
  WideWaveList list(slots, reinterpret_cast<int*>(slots + a.cap), lane, a.k, a.cap);
  cells_scan_body<D4>(a, list, lane, wave, q);
}

template <int D4>
struct WideCells {
  static constexpr auto kernel = &knn_cells_wide_kernel<D4>;
};

}  // namespace

}  // namespace mgp

extern "C" int mgp_knn_cells_wide_max_nn_count(void) { return mgp::kCellWideMaxK; }

extern "C" int mgp_knn_cells_scan_wide(const float* table, int64_t n, int d, const int64_t* cell_start, int nlist,
                                       const float* queries, int64_t m, const int32_t* probes, int nprobe,
                                       const int64_t* self_pos, int k, float* best_d, int32_t* best_i,
                                       int32_t* short_flag, void* stream) {
  using namespace mgp;
  if (n < 0 || m < 0 || d < 1 || k < 1 || nlist < 1 || nprobe < 1 || nprobe > nlist) return MGP_EINVAL;
  if (m == 0) return MGP_OK;
  if (!table || !cell_start || !queries || !probes || !best_d || !best_i || !short_flag) return MGP_EINVAL;
  if (d % 4 != 0 || d > 64 || k > kCellWideMaxK || n >= ((int64_t)1 << 31) ||
      (m + kCellWaves - 1) / kCellWaves >= ((int64_t)1 << 31))
    return MGP_EUNSUPPORTED;
  if (((uintptr_t)table | (uintptr_t)queries) % 16 != 0) return MGP_EUNSUPPORTED;
  const CellWideArgs a{{table, cell_start, queries, probes, self_pos, best_d, best_i, short_flag, n, m, nlist, nprobe, k},
                       wide_list_slots(k)};
  const size_t lds = (size_t)kCellWaves * a.cap * (sizeof(float) + sizeof(int));  // <= 48 KiB: no attribute needed
  return launch_cells_d4<WideCells>(d / 4, a, lds, static_cast<hipStream_t>(stream));
}
