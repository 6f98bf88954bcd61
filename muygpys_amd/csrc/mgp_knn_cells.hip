// Approximate k-NN over an inverted-cell (IVF) index: the per-query scan of the probed cells.
//
// The table is stored cell by cell (k-means cells, muygpys_amd/neighbors.py); a query looks only at the rows of its
// `nprobe` nearest cells.  One wave serves one query; the four waves of a workgroup are independent (no barrier, no
// shared state, no workgroup waits on another, no atomics).
//
//   scan    per step every lane takes one row of the current cell -- the 64 rows of a step are one contiguous block of
//           64 d floats, read in 16-byte pieces -- and measures it against the query in the difference form, fp32 (the
//           form mgp_knn_finish_f32 re-measures in: nothing cancels).  The query row sits in scalar registers (its
//           address is wave-uniform; past d = 32 in LDS, read as a broadcast).  The rows of the next step are requested before the current ones are compared.
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
#include "mgp_knn_list.h"

namespace mgp {

namespace {

struct CellScanArgs {
  const float* table;
  const int64_t* cell_start;
  const float* queries;
  const int* probes;
  const int64_t* self_pos;
  float* best_d;
  int* best_i;
  int* short_flag;
  int64_t n, m;
  int nlist, nprobe, k;
};

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

  // the query row: its address is wave-uniform -> scalar registers up to d = 32; longer rows would spill those and are
  // broadcast from LDS instead (every lane reads the same 16 bytes: no bank conflict)
  constexpr bool QLDS = D4 > 8;
  __shared__ float4 s_query[QLDS ? kCellWaves : 1][QLDS ? D4 : 1];
  float4 qreg[QLDS ? 1 : D4];
  {
    const float4* qr = reinterpret_cast<const float4*>(a.queries + q * (int64_t)(4 * D4));
    if constexpr (QLDS) {
      if (lane < D4) s_query[wave][lane] = qr[lane];
      wave_lds_fence();
    } else {
#pragma unroll
      for (int c = 0; c < D4; ++c) qreg[c] = qr[c];
    }
  }
  const int64_t self = a.self_pos ? a.self_pos[q] : (int64_t)-1;
  const int* pr = a.probes + q * (int64_t)a.nprobe;

  // the steps of the scan: (first row, end of its cell), cell after cell
  int pi = 0;
  int64_t r = 0, e = 0;
  auto next_step = [&]() -> bool {
    while (r >= e) {
      if (pi >= a.nprobe) return false;
      const int c = pr[pi++];
      if (c < 0 || c >= a.nlist) continue;
      r = a.cell_start[c];
      e = a.cell_start[c + 1];
      if (r < 0) r = 0;
      if (e > a.n) e = a.n;
    }
    return true;
  };
  auto load_rows = [&](float4 (&x)[D4], int64_t& row) {
    row = r + lane;
    const int64_t at = row < e ? row : e - 1;  // (lanes past the end of the cell read its last row and drop it)
    const float4* xr = reinterpret_cast<const float4*>(a.table + at * (int64_t)(4 * D4));
#pragma unroll
    for (int c = 0; c < D4; ++c) x[c] = xr[c];
  };

  float4 cur[D4], nxt[D4];
  int64_t cur_row = 0, nxt_row = 0, cur_end = 0;
  bool have = next_step();
  if (have) {
    load_rows(cur, cur_row);
    cur_end = e;
    r += 64;
  }
  while (have) {
    const bool have_next = next_step();
    int64_t nxt_end = 0;
    if (have_next) {
      load_rows(nxt, nxt_row);
      nxt_end = e;
      r += 64;
    }
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
#pragma unroll
    for (int c = 0; c < D4; ++c) {
      float4 qc;
      if constexpr (QLDS) qc = s_query[wave][c];
      else qc = qreg[c];
      const float e0 = qc.x - cur[c].x, e1 = qc.y - cur[c].y, e2 = qc.z - cur[c].z, e3 = qc.w - cur[c].w;
      s0 = __builtin_fmaf(e0, e0, s0);
      s1 = __builtin_fmaf(e1, e1, s1);
      s2 = __builtin_fmaf(e2, e2, s2);
      s3 = __builtin_fmaf(e3, e3, s3);
    }
    const float dd = (s0 + s1) + (s2 + s3);
    list.admit(cur_row < cur_end && cur_row != self && dd <= list.tau, dd, cur_row);
    have = have_next;
    if (have_next) {
#pragma unroll
      for (int c = 0; c < D4; ++c) cur[c] = nxt[c];
      cur_row = nxt_row;
      cur_end = nxt_end;
    }
  }
  if (list.npend > 0) list.merge();

  list.store(a.best_d, a.best_i, q);
  if (lane == 0) a.short_flag[q] = list.held < a.k ? 1 : 0;
}

template <int D4>
int launch_cells(const CellScanArgs& a, hipStream_t s) {
  const unsigned grid = (unsigned)((a.m + kCellWaves - 1) / kCellWaves);
  hipLaunchKernelGGL(knn_cells_scan_kernel<D4>, dim3(grid), dim3(kCellWaves * 64), 0, s, a);
  MGP_HIP_CHECK_LAUNCH();
  return MGP_OK;
}

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
  hipStream_t s = static_cast<hipStream_t>(stream);
  switch (d / 4) {
#define MGP_CELLS(V) \
  case V:            \
    return launch_cells<V>(a, s);
    MGP_CELLS(1) MGP_CELLS(2) MGP_CELLS(3) MGP_CELLS(4) MGP_CELLS(5) MGP_CELLS(6) MGP_CELLS(7) MGP_CELLS(8)
    MGP_CELLS(9) MGP_CELLS(10) MGP_CELLS(11) MGP_CELLS(12) MGP_CELLS(13) MGP_CELLS(14) MGP_CELLS(15) MGP_CELLS(16)
#undef MGP_CELLS
  }
  return MGP_EUNSUPPORTED;
}
