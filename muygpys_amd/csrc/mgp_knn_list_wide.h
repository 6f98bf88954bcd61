// The k-best list of ONE WAVE in LDS for lists wider than a wave (mgp_knn_cells_wide.hip: the probed cells of the
// inverted-cell index at 1 <= k <= 1024).  mgp_knn_list.h keeps its list in three registers per lane; up to 24 entries
// per lane do not fit next to two row buffers of d = 64, so here the entries stay in LDS and every pass re-reads them.
//
//   slots   cap = LW + P of them, LW = 64 ceil(k / 64), P = max(128, 64 ceil(LW / 128)) (wide_list_slots); the entries
//           are ONE contiguous run [0, total): the list first, what was admitted since the last selection behind it.
//   admit   a row at or below the wave-uniform threshold tau appends (distance, position) at `total` by ballot and
//           prefix count.  Until the slots run out nothing is selected -- tau stays +inf while total <= k, and filling
//           the list costs no pass at all (the narrow merge() runs its bisection even then).
//   select  when another full step might not fit (total > cap - 64), or at the end with total > k: the k-th smallest
//           key by bisection on the 32 bits of float_key, the counts by ballot over ceil(total / 64) slot groups read
//           from LDS four at a time; entries tied at the k-th distance are taken in order of stored position (a
//           second bisection, on the position bits, only when such a tie exists).  The chosen k are compacted IN
//           PLACE in ascending slot order: a group is read whole before any of it is written, and an entry's
//           destination is never ahead of its source.  The result is the k smallest by (distance, position) of the
//           candidate set, whatever the order the candidates came in.
//
// Nothing here synchronises beyond the wave: the owner hands every wave its own slots.
#pragma once

#include <cstdint>

#include "mgp_knn_list.h"

namespace mgp {

constexpr int kCellWideMaxK = 1024;

// (list slots + pending slots) of one wave at this k: a multiple of 64, at most 1536 (12 KiB of LDS with the positions)
__host__ __device__ inline int wide_list_slots(int k) {
  const int lw = (k + 63) / 64 * 64;
  const int p = (lw + 127) / 128 * 64;
  return lw + (p < 128 ? 128 : p);
}

struct WideWaveList {
  float* ld;  // cap distances of this wave (LDS)
  int* lp;    // ... and stored positions
  int lane;
  unsigned long long lanes_below;
  int k, cap;
  int total = 0;  // entries held (wave-uniform): at most k right after a selection
  float tau = __builtin_inff();

  __device__ __forceinline__ WideWaveList(float* dist, int* pos, int lane_, int k_, int cap_)
      : ld(dist), lp(pos), lane(lane_), lanes_below((1ull << lane_) - 1ull), k(k_), cap(cap_) {}

  // number of entries with key < trial (an admitted distance is never NaN: no entry carries the key of an empty slot)
  __device__ __forceinline__ int count_below(unsigned trial, int groups) const {
    int cnt = 0;
#pragma unroll 1
    for (int g = 0; g < groups; g += 4) {
      unsigned key[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int s = (g + j) * 64 + lane;
        key[j] = s < total ? cell_key(ld[s]) : 0xFFFFFFFFu;
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) cnt += popc64(__ballot(key[j] < trial));
    }
    return cnt;
  }

  // the k smallest of the `total` > k entries by (distance, position) -> slots [0, k)
  __device__ __forceinline__ void select() {
    const int groups = (total + 63) >> 6;
    // T = the k-th smallest key: the largest T with count(key < T) < k
    unsigned T = 0;
#pragma unroll 1
    for (int bit = 31; bit >= 0; --bit) {
      const unsigned trial = T | (1u << bit);
      if (count_below(trial, groups) < k) T = trial;
    }
    const int need = k - count_below(T, groups);  // >= 1 of the entries at T
    int equal = 0;
#pragma unroll 1
    for (int g = 0; g < groups; ++g) {
      const int s = g * 64 + lane;
      equal += popc64(__ballot(s < total && cell_key(ld[s]) == T));
    }
    int P = 0x7FFFFFFF;  // the largest position taken among them
    if (equal > need) {
      P = 0;
#pragma unroll 1
      for (int bit = 30; bit >= 0; --bit) {
        const int trial = P | (1 << bit);
        int cnt = 0;
#pragma unroll 1
        for (int g = 0; g < groups; ++g) {
          const int s = g * 64 + lane;
          cnt += popc64(__ballot(s < total && cell_key(ld[s]) == T && lp[s] < trial));
        }
        if (cnt < need) P = trial;
      }
    }
    int base = 0;
#pragma unroll 1
    for (int g = 0; g < groups; ++g) {
      const int s = g * 64 + lane;
      const bool on = s < total;
      const float dv = on ? ld[s] : 0.f;
      const int pv = on ? lp[s] : 0;
      const unsigned key = cell_key(dv);
      const bool sel = on && (key < T || (key == T && pv <= P));
      const unsigned long long mask = __ballot(sel);
      const int at = base + popc64(mask & lanes_below);  // <= s
      wave_lds_fence();                                  // (the whole group is read before any of it is written)
      if (sel && at < k) {
        ld[at] = dv;
        lp[at] = pv;
      }
      wave_lds_fence();
      base += popc64(mask);
    }
    total = k;
    tau = cell_unkey(T);
  }

  // one step of the scan: the lanes that `pass` append (dd, row); selected once another full step might not fit
  __device__ __forceinline__ void admit(bool pass, float dd, int64_t row) {
    const unsigned long long mask = __ballot(pass);
    if (mask) {
      if (pass) {
        const int at = total + popc64(mask & lanes_below);  // < cap: total <= cap - 64 between steps
        ld[at] = dd;
        lp[at] = (int)row;
      }
      total += popc64(mask);
      wave_lds_fence();
      if (total > cap - 64) select();
    }
  }

  // after the last step
  __device__ __forceinline__ void finish() {
    if (total > k) select();
  }
  __device__ __forceinline__ int filled() const { return total; }

  // the list -> row q of best_d / best_i (m, k): +inf / -1 in the slots the candidates did not fill
  __device__ __forceinline__ void store(float* best_d, int* best_i, int64_t q) const {
#pragma unroll 1
    for (int s = lane; s < k; s += 64) {
      const bool on = s < total;
      best_d[q * k + s] = on ? ld[s] : __builtin_inff();
      best_i[q * k + s] = on ? lp[s] : -1;
    }
  }
};

}  // namespace mgp
