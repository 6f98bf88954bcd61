// The k-best list of ONE WAVE in LDS, shared by the per-query scans (mgp_knn_cells.hip: the probed cells of the
// inverted-cell index; mgp_knn_grid.hip: the shells of the grid walk): 64 list slots, 128 pending slots behind them.
//
//   admit   a row at or below the wave-uniform threshold tau (the running k-th best; +inf until k rows are held)
//           appends (distance, position) to the pending slots by ballot and prefix count.
//   merge   the k smallest of list + pending are selected the way topk_rows_kernel does it (mgp_knn_select.hip:
//           bisection on the 32 bits of float_key), the counts by ballot; entries tied at the k-th distance are taken
//           in order of stored position (a second bisection, on the position bits, only when such a tie exists).  The
//           result is therefore the k smallest by (distance, position) of the candidate set, whatever the order the
//           candidates came in.
//
// Nothing here synchronises beyond the wave: the owner hands every wave its own slots.
#pragma once

#include <cstdint>

namespace mgp {

constexpr int kCellWaves = 4;     // queries per workgroup
constexpr int kCellList = 64;     // list slots per wave (k <= 64)
constexpr int kCellPending = 128; // pending slots per wave: merged when fewer than 64 are free
constexpr int kCellSlots = kCellList + kCellPending;

__device__ __forceinline__ unsigned cell_key(float x) {  // float_key of mgp_knn_select.hip
  const unsigned u = __float_as_uint(x);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float cell_unkey(unsigned key) {
  return __uint_as_float((key & 0x80000000u) ? (key ^ 0x80000000u) : ~key);
}
__device__ __forceinline__ int popc64(unsigned long long m) { return __builtin_popcountll(m); }
// the LDS traffic of one wave is in program order; this keeps the compiler from moving it
__device__ __forceinline__ void wave_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

struct WaveList {
  float* ld;  // kCellSlots distances of this wave (LDS)
  int* lp;    // ... and stored positions
  int lane;
  unsigned long long lanes_below;
  int k;
  int held = 0, npend = 0;  // entries of the list / of the pending slots (wave-uniform)
  float tau = __builtin_inff();

  __device__ __forceinline__ WaveList(float* dist, int* pos, int lane_, int k_)
      : ld(dist), lp(pos), lane(lane_), lanes_below((1ull << lane_) - 1ull), k(k_) {}

  // the k smallest of list + pending by (distance, position) -> list
  __device__ __forceinline__ void merge() {
    const int total = held + npend;
    const int kk = total < k ? total : k;
    unsigned key[3];
    float dv[3];
    int pv[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int s = j * 64 + lane;
      const bool on = j == 0 ? s < held : (s - kCellList) < npend;
      dv[j] = ld[s];
      pv[j] = lp[s];
      key[j] = on ? cell_key(dv[j]) : 0xFFFFFFFFu;  // (an admitted distance is never NaN: no entry carries this key)
    }
    wave_lds_fence();
    // T = the kk-th smallest key: the largest T with count(key < T) < kk
    unsigned T = 0;
#pragma unroll 1
    for (int bit = 31; bit >= 0; --bit) {
      const unsigned trial = T | (1u << bit);
      const int cnt = popc64(__ballot(key[0] < trial)) + popc64(__ballot(key[1] < trial)) + popc64(__ballot(key[2] < trial));
      if (cnt < kk) T = trial;
    }
    const int below = popc64(__ballot(key[0] < T)) + popc64(__ballot(key[1] < T)) + popc64(__ballot(key[2] < T));
    const int equal = popc64(__ballot(key[0] == T)) + popc64(__ballot(key[1] == T)) + popc64(__ballot(key[2] == T));
    const int need = kk - below;  // >= 1 of the `equal` entries at T
    int P = 0x7FFFFFFF;           // the largest position taken among them
    if (equal > need) {
      P = 0;
#pragma unroll 1
      for (int bit = 30; bit >= 0; --bit) {
        const int trial = P | (1 << bit);
        const int cnt = popc64(__ballot(key[0] == T && pv[0] < trial)) + popc64(__ballot(key[1] == T && pv[1] < trial)) +
                        popc64(__ballot(key[2] == T && pv[2] < trial));
        if (cnt < need) P = trial;
      }
    }
    int base = 0;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const bool sel = key[j] < T || (key[j] == T && pv[j] <= P);
      const unsigned long long mask = __ballot(sel);
      const int at = base + popc64(mask & lanes_below);
      if (sel && at < kk) {
        ld[at] = dv[j];
        lp[at] = pv[j];
      }
      base += popc64(mask);
    }
    wave_lds_fence();
    held = kk;
    npend = 0;
    if (total >= k) tau = cell_unkey(T);
  }

  // one step of the scan: the lanes that `pass` append (dd, row); merged once another full step might not fit
  __device__ __forceinline__ void admit(bool pass, float dd, int64_t row) {
    const unsigned long long mask = __ballot(pass);
    if (mask) {
      if (pass) {
        const int at = kCellList + npend + popc64(mask & lanes_below);
        ld[at] = dd;
        lp[at] = (int)row;
      }
      npend += popc64(mask);
      wave_lds_fence();
      if (npend > kCellPending - 64) merge();
    }
  }

  // the list -> row q of best_d / best_i (m, k): +inf / -1 in the slots the candidates did not fill
  __device__ __forceinline__ void store(float* best_d, int* best_i, int64_t q) const {
    if (lane < k) {
      const bool on = lane < held;
      best_d[q * k + lane] = on ? ld[lane] : __builtin_inff();
      best_i[q * k + lane] = on ? lp[lane] : -1;
    }
  }
};

}  // namespace mgp
