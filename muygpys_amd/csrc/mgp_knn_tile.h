// The 64-row MFMA tile that knn_scan_kernel (mgp_knn.hip), knn_scan_wide_kernel (mgp_knn_wide.hip) and
// knn_cells_block_kernel (mgp_knn_cells_block.hip) are built on: a wave of lanes (r32 = lane % 32, half = lane / 32)
// holds 32 query rows as the A operand, a tile of KNN_TN table rows is staged in LDS at a row stride of DP + 4 floats
// (an odd number of 16-byte slots), and two chains of v_mfma_f32_32x32x2_f32 give  q.x - |x|^2/2  for 32 x 64 pairs.
// Here: the staging passes and the accumulator-row map.  The A-operand load and the two-block Gram step stay written
// out in each kernel: as functions of this header they changed the code of the DP = 8 instantiations (30 instructions
// of knn_scan_kernel<8>, one SGPR of knn_cells_block_kernel<8>), and the kernels' speed is not this header's to move.
// How the norms arrive, the survivor queues, the drains and the tile walk differ between the kernels and are theirs.
#pragma once

#include "mgp_knn_common.h"

namespace mgp {

// accumulator register v of a lane belongs to this query row of the wave.  (Where a kernel adds the wave's first slot,
// w KNN_QW + 8 (v/4) + 4 half + v%4, the sum stays written out left to right: through this function the compiler
// associates it differently and the kernel's address arithmetic changes.)
constexpr int tile_acc_row(int v, int half) { return 8 * (v >> 2) + 4 * half + (v & 3); }

// Staging with direct global->LDS loads, wave w's share of the rows of one tile: a wave-instruction fills 64 consecutive
// 16-byte slots; slot sigma of a tile is row sigma / SPR, column sigma % SPR (the padding column and the columns past d
// repeat the row's last data slot -- finite values the zero-padded query operand cancels).  Rows past n repeat row
// n - 1: the caller masks them by their norm.  dslots = d / 4, divided once by the caller.
template <int DP>
__device__ __forceinline__ void tile_stage_rows(float* tile, const float* table, int64_t n, int d, int dslots, int64_t t0, int w,
                                                int lane) {
  constexpr int SPR = (DP + 4) / 4;
  constexpr int NPASS = (KNN_TN * SPR + 63) / 64;
  for (int p = w; p < NPASS; p += 4) {
    const int sigma = 64 * p + lane;
    const int row = min(sigma / SPR, KNN_TN - 1);
    const int c = min(sigma - row * SPR, dslots - 1);
    const int64_t grow = min(t0 + row, n - 1);
    lds_dma16(table + grow * (int64_t)d + c * 4, lds_offset(tile) + p * 1024);
  }
}

}  // namespace mgp
