// Approximate k-NN over an inverted-cell (IVF) index for k-best lists WIDER THAN A WAVE: the per-query scan of the
// probed cells at 1 <= k <= 1024 (mgp_knn_cells.hip stops at 64, the width of its register-held list).
//
// One wave serves one query; the four waves of a workgroup are independent (no barrier, no shared state, no workgroup
// waits on another, no atomics).
//
//   scan    mgp_knn_cells.hip's: per step every lane takes one row of the current cell -- 64 contiguous rows, read in
//           16-byte pieces -- and measures it against the query in the difference form, fp32, four partial sums added
//           as (s0 + s1) + (s2 + s3): at equal k both kernels return the same bits.  The query row sits in scalar
//           registers (past d = 32 in LDS, read as a broadcast); the rows of the next step are requested before the
//           current ones are compared.
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
#include "mgp_knn_list_wide.h"

namespace mgp {

namespace {

struct CellWideArgs {
  const float* table;
  const int64_t* cell_start;
  const float* queries;
  const int* probes;
  const int64_t* self_pos;
  float* best_d;
  int* best_i;
  int* short_flag;
  int64_t n, m;
  int nlist, nprobe, k, cap;
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
  if (lane == 0) a.short_flag[q] = list.total < a.k ? 1 : 0;
}

template <int D4>
int launch_cells_wide(const CellWideArgs& a, hipStream_t s) {
  const unsigned grid = (unsigned)((a.m + kCellWaves - 1) / kCellWaves);
  const size_t lds = (size_t)kCellWaves * a.cap * (sizeof(float) + sizeof(int));  // <= 48 KiB: no attribute needed
  hipLaunchKernelGGL(knn_cells_wide_kernel<D4>, dim3(grid), dim3(kCellWaves * 64), lds, s, a);
  MGP_HIP_CHECK_LAUNCH();
  return MGP_OK;
}

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
  const CellWideArgs a{table,      cell_start, queries, probes, self_pos, best_d, best_i,
                       short_flag, n,          m,       nlist,  nprobe,   k,      wide_list_slots(k)};
  hipStream_t s = static_cast<hipStream_t>(stream);
  switch (d / 4) {
#define MGP_CELLS_WIDE(V) \
  case V:                 \
    return launch_cells_wide<V>(a, s);
    MGP_CELLS_WIDE(1) MGP_CELLS_WIDE(2) MGP_CELLS_WIDE(3) MGP_CELLS_WIDE(4) MGP_CELLS_WIDE(5) MGP_CELLS_WIDE(6)
    MGP_CELLS_WIDE(7) MGP_CELLS_WIDE(8) MGP_CELLS_WIDE(9) MGP_CELLS_WIDE(10) MGP_CELLS_WIDE(11) MGP_CELLS_WIDE(12)
    MGP_CELLS_WIDE(13) MGP_CELLS_WIDE(14) MGP_CELLS_WIDE(15) MGP_CELLS_WIDE(16)
#undef MGP_CELLS_WIDE
  }
  return MGP_EUNSUPPORTED;
}
