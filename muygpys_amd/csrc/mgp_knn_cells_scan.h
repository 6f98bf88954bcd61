// The per-query scan of the probed cells of the inverted-cell index, written once for both list widths:
// knn_cells_scan_kernel (mgp_knn_cells.hip, WaveList, k <= 64) and knn_cells_wide_kernel (mgp_knn_cells_wide.hip,
// WideWaveList, k <= 1024) carve their LDS, build their list and call cells_scan_body.  One copy of the arithmetic:
// at equal k both kernels return the same bits.
//
//   scan    per step every lane takes one row of the current cell -- the 64 rows of a step are one contiguous block of
//           64 d floats, read in 16-byte pieces -- and measures it against the query in the difference form, fp32, four
//           partial sums added as (s0 + s1) + (s2 + s3) (the form mgp_knn_finish_f32 re-measures in: nothing cancels).
//           The query row sits in scalar registers (its address is wave-uniform; past d = 32 in LDS, read as a
//           broadcast).  The rows of the next step are requested before the current ones are compared.
//   list    any type with tau, admit(pass, distance, row), finish(), filled() and store(best_d, best_i, q)
//           (mgp_knn_list.h, mgp_knn_list_wide.h).
#pragma once

#include <cstdint>

#include "mgp_args.h"
#include "mgp_knn_list.h"

namespace mgp {

namespace {  // (the kernels' argument type: internal to each of the two translation units, like the kernels)

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

// D4 = d / 4; query q is this wave's
template <int D4, class List>
__device__ __forceinline__ void cells_scan_body(const CellScanArgs& a, List& list, int lane, int wave, int64_t q) {
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
  list.finish();

  list.store(a.best_d, a.best_i, q);
  if (lane == 0) a.short_flag[q] = list.filled() < a.k ? 1 : 0;
}

// One workgroup of kCellWaves waves per kCellWaves queries, the instantiation by row width: K<D4>::kernel is the
// __global__ function for rows of 4 D4 floats (D4 = 1 .. 16)
template <template <int> class K, class Args>
int launch_cells_d4(int d4, const Args& a, size_t lds, hipStream_t s) {
  const dim3 grid((unsigned)((a.m + kCellWaves - 1) / kCellWaves)), block(kCellWaves * 64);
  switch (d4) {
#define MGP_CELLS(V)                                             \
  case V:                                                        \
    hipLaunchKernelGGL(K<V>::kernel, grid, block, lds, s, a); \
    break;
    MGP_CELLS(1) MGP_CELLS(2) MGP_CELLS(3) MGP_CELLS(4) MGP_CELLS(5) MGP_CELLS(6) MGP_CELLS(7) MGP_CELLS(8)
    MGP_CELLS(9) MGP_CELLS(10) MGP_CELLS(11) MGP_CELLS(12) MGP_CELLS(13) MGP_CELLS(14) MGP_CELLS(15) MGP_CELLS(16)
#undef MGP_CELLS
    default:
      return MGP_EUNSUPPORTED;
  }
  MGP_HIP_CHECK_LAUNCH();
  return MGP_OK;
}

}  // namespace

}  // namespace mgp
