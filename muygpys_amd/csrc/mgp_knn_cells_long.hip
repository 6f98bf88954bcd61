// Approximate k-NN over an inverted-cell (IVF) index for LONG ROWS: the per-query scan of the probed cells at
// d % 4 == 0, 68 <= d <= 256 (mgp_knn_cells.hip and mgp_knn_cells_wide.hip stop at d = 64: cells_scan_body holds the
// current and the prefetched row of every lane in registers, 2 d / 4 float4 -- 512 VGPRs at d = 256).
//
// One wave serves one query; the four waves of a workgroup are independent (no barrier, no shared state, no workgroup
// waits on another, no atomics).  The query row (at most 1 KiB) sits in the wave's LDS and is read as a broadcast.
//
//   rows    per step every lane takes one row of the current cell, as in cells_scan_body, but meets it in CHUNKS of
//           kLongChunk = 8 float4 (128 bytes, one cache line).  Only one chunk and its prefetch are in registers; the
//           four partial sums s0 .. s3 carry across the chunks of a step and the distance is (s0 + s1) + (s2 + s3) after
//           the last one -- the form mgp_knn_finish_f32 re-measures in.  The stored width stays d, not a multiple of the
//           chunk: the tail of d / 4 % 8 float4 (a run-time length) is the LAST chunk of a step, loaded as the row's
//           final 8 float4 -- it overlaps the chunk before it, and the overlapped slots are not added again.  Every
//           piece of the scan is therefore the same eight 16-byte loads at constant offsets, whatever d is, and the
//           compiler's count of loads in flight is exact on every path: the wait before a chunk is compared leaves the
//           prefetch behind it outstanding.
//   prune   after every chunk but the last the wave asks  __ballot(alive && (s0 + s1) + (s2 + s3) <= tau).  If no lane
//           can still enter the list the remaining chunks of the step are not read.  This is EXACT, not a heuristic:
//           each s_i is a monotone fp32 sequence -- fma(e, e, s) >= s for the non-negative e e, rounding is monotone and
//           s is representable -- and (s0 + s1) + (s2 + s3) is monotone in each argument, so the value after a chunk is
//           a lower bound of the value after the last one, bit for bit.  A row dropped at a chunk has a full distance
//           above tau and admit() would have refused it (a NaN partial sum stays NaN and is refused either way); tau
//           does not move inside a step.  The result equals the unpruned scan's, bit for bit.  While the list is
//           unfilled tau = +inf and nothing is pruned.
//   fetch   the next piece -- the same step's next chunk, else chunk 0 of the next step, of the next cell at a cell's
//           end -- is requested before the current one is compared, into the other of two register buffers (the loop
//           is unrolled by two: no copies).  A prefetch a prune made useless is dropped and chunk 0 of the next step
//           read in its place.  After the last piece the request repeats chunk 0 of the last step (valid memory).
//   ends    lanes past a cell's end read its last row and are not alive; the row `self_pos` is not alive either.
//   list    k <= 64: WaveList (mgp_knn_list.h), static LDS; k <= 1024: WideWaveList (mgp_knn_list_wide.h), dynamic LDS
//           of wide_list_slots(k) slots per wave, as knn_cells_wide_kernel -- both used as they are.
//
// Resources (lib/kernel_resources.json; tests/test_knn_cells_long_status_cpu.py reads the records):
//
//   kernel                      VGPRs  SGPRs  static LDS  dynamic LDS      waves/SIMD  VGPR spill  scratch
//   cells_longrow_kernel            93     99    10 240 B    0                    5           0         0
//   cells_longrow_wide_kernel       98    100     4 096 B    8 .. 48 KiB          4           0         0
//
// (waves/SIMD as the registers allow: two chunk buffers are 64 of them.  A workgroup is one wave per SIMD, so LDS bounds
// the wide form at k = 1024 to three workgroups per CU -- 52 KiB each; up to k = 704 (38.8 KiB) and in the narrow form
// the registers are the bound.)
//
// Reference: the approximate branch of the reference's neighbour search (hnswlib behind NN_Wrapper,
// src/MuyGPyS/neighbors.py:109-127,213-262) takes any feature count; its torch tutorial searches a 100-dimensional
// embedding.
#include <cstdint>

#include "mgp_args.h"
#include "mgp_knn_cells_scan.h"
#include "mgp_knn_list_wide.h"

// A/B builds only (tools/mkvariant.sh): the scan without the chunk-wise prune test
#ifndef MGP_CELLS_LONG_PRUNE
#define MGP_CELLS_LONG_PRUNE 1
#endif

namespace mgp {

namespace {

constexpr int kLongChunk = 8;                    // float4 per chunk: 128 bytes
constexpr int kLongMaxD4 = KNN_LONG_MAX_D / 4;  // float4 per query row, at most
static_assert(kLongMaxD4 <= 64, "a wave stages its query row in one pass");

struct CellLongArgs : CellScanArgs {
  int d4;   // d / 4: 17 .. 64
  int cap;  // wide_list_slots(k) (the wide list only)
};

// query q is this wave's, `sq` its kLongMaxD4 float4 of LDS
template <class List>
__device__ __forceinline__ void cells_longrow_body(const CellLongArgs& a, List& list, float4* sq, int lane, int64_t q) {
  constexpr int CH = kLongChunk;
  const int d4 = a.d4;
  const int nfull = d4 / CH, t4 = d4 % CH;
  const int nch = nfull + (t4 ? 1 : 0);  // chunks per step: >= 3
  {
    const float4* qr = reinterpret_cast<const float4*>(a.queries + q * (int64_t)(4 * d4));
    if (lane < d4) sq[lane] = qr[lane];
    wave_lds_fence();
  }
  const int64_t self = a.self_pos ? a.self_pos[q] : (int64_t)-1;
  const int* pr = a.probes + q * (int64_t)a.nprobe;

  // the steps of the scan: (first row, end of its cell), cell after cell
  int pi = 0;
  int64_t r = 0, e = 0;
  auto take_step = [&](int64_t& first, int64_t& end) -> bool {
    while (r >= e) {
      if (pi >= a.nprobe) return false;
      const int c = pr[pi++];
      if (c < 0 || c >= a.nlist) continue;
      r = a.cell_start[c];
      e = a.cell_start[c + 1];
      if (r < 0) r = 0;
      if (e > a.n) e = a.n;
    }
    first = r;
    end = e;
    r += 64;
    return true;
  };
  // chunk ci of the step: float4 [ci CH, ci CH + CH) of the lane's row; the tail is the row's last CH float4
  auto load_piece = [&](float4 (&x)[CH], int64_t first, int64_t end, int ci) {
    const int64_t row = first + lane;
    const int64_t at = row < end ? row : end - 1;  // (lanes past the end of the cell read its last row and drop it)
    const int c0 = ci < nfull ? ci * CH : d4 - CH;
    const float4* xr = reinterpret_cast<const float4*>(a.table + at * (int64_t)(4 * d4)) + c0;
#pragma unroll
    for (int c = 0; c < CH; ++c) x[c] = xr[c];
  };

  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  auto add_slot = [&](const float4& qc, const float4& xc) {
    const float e0 = qc.x - xc.x, e1 = qc.y - xc.y, e2 = qc.z - xc.z, e3 = qc.w - xc.w;
    s0 = __builtin_fmaf(e0, e0, s0);
    s1 = __builtin_fmaf(e1, e1, s1);
    s2 = __builtin_fmaf(e2, e2, s2);
    s3 = __builtin_fmaf(e3, e3, s3);
  };

  // the piece in hand: chunk ci of the step whose rows start at `first`, in a cell that ends at `end`
  int64_t first = 0, end = 0;
  int ci = 0;
  // compares the piece in `cur` after requesting the one behind it into `nxt`; false after the last piece
  auto piece = [&](float4 (&cur)[CH], float4 (&nxt)[CH]) -> bool {
    int64_t nfirst = first, nend = end;
    int nci = ci + 1;
    bool more = true;
    if (nci == nch) {
      more = take_step(nfirst, nend);  // (none left: chunk 0 of this step again, dropped)
      nci = 0;
    }
    load_piece(nxt, nfirst, nend, nci);
    if (ci < nfull) {
      const float4* qc = sq + ci * CH;
#pragma unroll
      for (int c = 0; c < CH; ++c) add_slot(qc[c], cur[c]);
    } else {  // the tail: its first CH - t4 slots were added with the chunk before
      const float4* qc = sq + (d4 - CH);
#pragma unroll
      for (int c = 1; c < CH; ++c)
        if (c >= CH - t4) add_slot(qc[c], cur[c]);  // (wave-uniform; t4 <= CH - 1)
    }
    const int64_t row = first + lane;
    const bool alive = row < end && row != self;
    const float dd = (s0 + s1) + (s2 + s3);
    if (ci == nch - 1) {
      list.admit(alive && dd <= list.tau, dd, row);
      s0 = s1 = s2 = s3 = 0.f;
    }
#if MGP_CELLS_LONG_PRUNE
    else if (!__ballot(alive && dd <= list.tau)) {
      // no lane of this step can enter the list any more: its remaining chunks are skipped
      s0 = s1 = s2 = s3 = 0.f;
      more = take_step(nfirst, nend);
      nci = 0;
      if (more) load_piece(nxt, nfirst, nend, 0);
    }
#endif
    first = nfirst, end = nend, ci = nci;
    return more;
  };

  float4 buf0[CH], buf1[CH];
  if (take_step(first, end)) {
    load_piece(buf0, first, end, 0);
    while (piece(buf0, buf1) && piece(buf1, buf0)) {
    }
  }
  list.finish();

  list.store(a.best_d, a.best_i, q);
  if (lane == 0) a.short_flag[q] = list.filled() < a.k ? 1 : 0;
}

// k <= 64
__global__ __launch_bounds__(kCellWaves * 64) void cells_longrow_kernel(const CellLongArgs a) {
  __shared__ float4 s_query[kCellWaves][kLongMaxD4];
  __shared__ float s_dist[kCellWaves][kCellSlots];
  __shared__ int s_pos[kCellWaves][kCellSlots];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t q = (int64_t)blockIdx.x * kCellWaves + wave;
  if (q >= a.m) return;
  WaveList list(s_dist[wave], s_pos[wave], lane, a.k);
  cells_longrow_body(a, list, s_query[wave], lane, q);
}

// k <= 1024
__global__ __launch_bounds__(kCellWaves * 64) void cells_longrow_wide_kernel(const CellLongArgs a) {
  extern __shared__ float4 s_slots[];  // per wave: cap distances, then cap positions
  __shared__ float4 s_query[kCellWaves][kLongMaxD4];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t q = (int64_t)blockIdx.x * kCellWaves + wave;
  if (q >= a.m) return;
  float* slots = reinterpret_cast<float*>(s_slots) + (size_t)wave * 2 * a.cap;
  WideWaveList list(slots, reinterpret_cast<int*>(slots + a.cap), lane, a.k, a.cap);
  cells_longrow_body(a, list, s_query[wave], lane, q);
}

}  // namespace

}  // namespace mgp

extern "C" int mgp_knn_cells_scan_long(const float* table, int64_t n, int d, const int64_t* cell_start, int nlist,
                                       const float* queries, int64_t m, const int32_t* probes, int nprobe,
                                       const int64_t* self_pos, int k, float* best_d, int32_t* best_i,
                                       int32_t* short_flag, void* stream) {
  using namespace mgp;
  if (n < 0 || m < 0 || d < 1 || k < 1 || nlist < 1 || nprobe < 1 || nprobe > nlist) return MGP_EINVAL;
  if (m == 0) return MGP_OK;
  if (!table || !cell_start || !queries || !probes || !best_d || !best_i || !short_flag) return MGP_EINVAL;
  if (d % 4 != 0 || d <= 64 || d > mgp_knn_long_max_features() || k > kCellWideMaxK || n >= ((int64_t)1 << 31) ||
      (m + kCellWaves - 1) / kCellWaves >= ((int64_t)1 << 31))
    return MGP_EUNSUPPORTED;
  if (((uintptr_t)table | (uintptr_t)queries) % 16 != 0) return MGP_EUNSUPPORTED;
  const bool wide = k > kCellList;
  const CellLongArgs a{{table, cell_start, queries, probes, self_pos, best_d, best_i, short_flag, n, m, nlist, nprobe, k},
                       d / 4, wide ? wide_list_slots(k) : 0};
  const dim3 grid((unsigned)((m + kCellWaves - 1) / kCellWaves)), block(kCellWaves * 64);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (wide) {
    // <= 48 KiB, 52 KiB with the query rows: no attribute needed
    const size_t lds = (size_t)kCellWaves * a.cap * (sizeof(float) + sizeof(int));
    hipLaunchKernelGGL(cells_longrow_wide_kernel, grid, block, lds, s, a);
  } else {
    hipLaunchKernelGGL(cells_longrow_kernel, grid, block, 0, s, a);
  }
  MGP_HIP_CHECK_LAUNCH();
  return MGP_OK;
}
