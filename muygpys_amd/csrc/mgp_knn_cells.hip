// Approximate k-NN over an inverted-cell (IVF) index: the per-query scan of the probed cells.
//
// The table is stored cell by cell (k-means cells, muygpys_amd/neighbors.py); a query looks only at the rows of its
// `nprobe` nearest cells.  One wave serves one query; the four waves of a workgroup are independent (no barrier, no
// shared state, no workgroup waits on another, no atomics).
//
//   scan    cells_scan_body (mgp_knn_cells_scan.h, shared with the wide-list form mgp_knn_cells_wide.hip): per step every
//           lane takes one row of the current cell and measures it against the query in the difference form, fp32.
//   admit   a row at or below the wave-uniform threshold tau (the running k-th best; +inf until k rows are held)
//           appends (distance, position) to the wave's pending buffer in LDS by ballot and prefix count.
//   merge   when the buffer cannot take another full step, the k smallest of list + pending are selected the way
//           topk_rows_kernel does it (mgp_knn_select.hip: bisection on the 32 bits of float_key), the counts by ballot;
//           entries tied at the k-th distance are taken in order of stored position (a second bisection, on the
//           position bits, only when such a tie exists).  The result is therefore the k smallest by (distance,
//           position) of the candidate set, whatever the order of the cells or the neighbours in the workgroup.
//           After the first few hundred rows merges are rare: a row beats tau with probability ~ k / rows seen.
//           (admit and merge live in mgp_knn_list.h: the grid walk of mgp_knn_grid.hip keeps its list the same way.)
//
// Reference: the approximate branch of the reference's neighbour search (hnswlib behind NN_Wrapper,
// src/MuyGPyS/neighbors.py:109-127,213-262); the inverted-cell index fills the same role on a GPU.
#include <cstdint>

#include "mgp_args.h"
#include "mgp_knn_cells_scan.h"

namespace mgp {

namespace {

// D4 = d / 4
template <int D4>
__global__ __launch_bounds__(kCellWaves * 64) void knn_cells_scan_kernel(const CellScanArgs a) {
  __shared__ float s_dist[kCellWaves][kCellSlots];
  __shared__ int s_pos[kCellWaves][kCellSlots];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t q = (int64_t)blockIdx.x * kCellWaves + wave;
  if (q >= a.m) return;
  WaveList list(s_dist[wave], s_pos[wave], lane, a.k);
  cells_scan_body<D4>(a, list, lane, wave, q);
}

template <int D4>
struct NarrowCells {
  static constexpr auto kernel = &knn_cells_scan_kernel<D4>;
};

}  // namespace

}  // namespace mgp

extern "C" int mgp_knn_cells_scan(const float* table, int64_t n, int d, const int64_t* cell_start, int nlist,
                                  const float* queries, int64_t m, const int32_t* probes, int nprobe,
                                  const int64_t* self_pos, int k, float* best_d, int32_t* best_i, int32_t* short_flag,
                                  void* stream) {
  using namespace mgp;
  if (n < 0 || m < 0 || d < 1 || k < 1 || nlist < 1 || nprobe < 1 || nprobe > nlist) return MGP_EINVAL;
  if (d % 4 != 0 || d > 64 || k > 64 || n >= ((int64_t)1 << 31) || (m + kCellWaves - 1) / kCellWaves >= ((int64_t)1 << 31))
    return MGP_EUNSUPPORTED;
  if (m == 0) return MGP_OK;
  if (!table || !cell_start || !queries || !probes || !best_d || !best_i || !short_flag) return MGP_EINVAL;
  if (((uintptr_t)table | (uintptr_t)queries) % 16 != 0) return MGP_EUNSUPPORTED;
  const CellScanArgs a{table, cell_start, queries, probes, self_pos, best_d, best_i, short_flag, n, m, nlist, nprobe, k};
  return launch_cells_d4<NarrowCells>(d / 4, a, 0, static_cast<hipStream_t>(stream));
}
