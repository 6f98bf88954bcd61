// Exact k-nearest-neighbour scan for k-best lists of up to 1 024 entries with a split-bf16 pre-filter (d <= 64).
//
// The lists of csrc/mgp_knn_wide.hip behind the pre-filter of knn_scan_bf16x3_kernel (csrc/mgp_knn.hip): the same packed
// table and packed queries (rows [hi(KP) | lo(KP)] in bf16, KP = 16 ceil((d + 2) / 16) = 16 .. 80, the last two slots
// (c, 1) in a table row and (1, -thr) in a query row, c = -|x|^2/2 + 2^-14 QMAX |x| raised by 2^-15 |c|), three
// v_mfma_f32_32x32x16_bf16 chains hi.hi + hi.lo + lo.hi, so the accumulator IS q.x + c - thr and a pair survives iff it is
// positive.  KP <= 80 is at most 240 products per accumulator: the 2^-14 of the short rows holds as derived there, and
// the kernel lowers thr by 2^-14 |thr| (neg_thr_split).  Every survivor is re-measured EXACTLY (fp32 difference form, the
// arithmetic of the narrow packed drain) before it meets a list: best_d IN / OUT and tau only ever hold exact distances.
//
//   A operand   the wave's 64 queries (two row blocks of 32), whole packed rows, in registers for the whole scan: lane
//               (r32, half) holds the 16-byte pieces 2 J + half, J < NQ = KP / 16, of the hi and of the lo part -- 8 NQ
//               registers per row block.  The -thr slot (KP - 1) is the upper half-word of the last register of the last
//               piece of the upper lanes; after a drain those lanes rewrite it in place.
//   table side  64-row tiles of whole packed rows at a row stride of KP / 4 + 1 sixteen-byte slots (odd: 32 consecutive
//               rows read conflict-free), two buffers.  REGISTER staging, not global_load_lds: the next tile is requested
//               with plain 16-byte loads right behind the barrier and written to the other buffer after this tile's
//               matrix instructions -- next to the other waves' matrix instructions an LDS-DMA instruction took a few
//               hundred cycles to issue in knn_scan_bf16x3_kernel, which measured faster this way at every row length;
//               2 to 6 registers per lane, dead before the drain.  Four waves x 64 queries = 256 queries per
//               workgroup, one barrier per tile; workgroup b starts at tile 7919 b mod ntiles and wraps (running indices).
//   queue       a ring of BIT MASKS: per query KNN_PW_WINDOW x 64 bits, bit (s, c) = "column c of the s-th tile of the
//               window passed", set with atomicOr by the wave that owns the query, and one word per query with bit s set
//               where slot s is not empty.  A survivor is a candidate for re-measurement: its approximate accumulator is
//               not kept, there is no counter and no position to claim, and a window cannot hold more survivors than it
//               has bits -- no queue can overflow whatever the order of the table; `overflow` is never written.
//               256 queries x 8 tiles x 8 B = 16 KB (the fp32 slots of knn_scan_wide_kernel: 32 KB for 128 queries).  The
//               window's first tile is wave-uniform state; slot s is tile (first + s) mod ntiles (the walk wraps once).
//   cadence     the window is drained when it is full, at the last tile, and otherwise every
//               clamp(rows_seen / MGP_KNN_CADENCE, one tile, the window) rows -- the rule of knn_scan_bf16x3_kernel,
//               where knn_scan_wide_kernel drains after every tile.  A stale tau only lets more candidates through to
//               the exact test: no result depends on the cadence.
//   drain       (wave-private state, no barrier) one LDS read finds the wave's queries with a non-empty window.  For
//               each, the wave holds the list's distances as ceil(k / 64) entries per lane (load_list; the next pending
//               query's list is requested before this one is merged); for each non-empty slot lane = column, and the
//               lanes whose bit is set, whose row is not the self row and lies below n re-measure it: sum (q - x)^2 in
//               16-byte loads.  Insertion is knn_scan_wide_kernel's replace-the-maximum under cd < tau: one cross-lane
//               maximum per accepted candidate, the first lane at tau overwrites that one entry in registers and in
//               global memory, the row numbers are never read.  Then tau goes back to LDS, the masks are cleared and
//               the upper lanes rewrite their -thr slots.
//
// Resources (lib/kernel_resources.json; tests/test_knn_wide_bf16_status_cpu.py compares this table with the report).
// Dynamic LDS = 2 tiles + 16 KB of masks + 2 KB of slot words and tau: two workgroups per CU and more at every KP.
//
//   kernel                        KP  VGPRs  AGPRs  waves/SIMD  VGPR spill  scratch  LDS bytes
//   knn_prefilter_wide_kernel     16    131      0       3           0         0      28672
//   knn_prefilter_wide_kernel     32    155      0       3           0         0      36864
//   knn_prefilter_wide_kernel     48    179      0       2           0         0      45056
//   knn_prefilter_wide_kernel     64    203      0       2           0         0      53248
//   knn_prefilter_wide_kernel     80    227      0       2           0         0      61440
//
// (24 to 29 SGPRs are spilled to VGPR lanes.  The survivors' LDS addresses are one base per lane and tile plus constant
// offsets: with an address per accumulator register the compiler kept 30 more VGPRs live and KP = 80 spilled one.)
#include <cstdint>

#include "mgp_args.h"
#include "mgp_knn_common.h"

namespace mgp {

constexpr int PW_W = KNN_PW_WINDOW;   // tiles per window of the mask ring
constexpr int PW_QW = 2 * KNN_QW;     // queries per wave: two row blocks
constexpr int PW_QB = 4 * PW_QW;      // queries per workgroup
static_assert(PW_W <= 32 && PW_QB == 256, "one slot word per query, one thread per query of the workgroup");

constexpr size_t pw_lds_bytes(int kp) {
  return 2 * KNN_TN * (4 * kp + 16) + (size_t)PW_QB * (2 * PW_W + 2) * sizeof(unsigned);
}

template <int KP>
__global__ __launch_bounds__(256, 2) void knn_prefilter_wide_kernel(KnnPackedArgs a) {
  constexpr int NQ = KP / 16;           // matrix steps per chain
  constexpr int RB = 4 * KP;            // bytes of a packed row
  constexpr int SPR = RB / 16 + 1;      // 16-byte slots of a staged row (odd) = wave passes per tile
  constexpr int XSB = SPR * 16;         // LDS row stride in bytes
  constexpr int IPW = (SPR + 3) / 4;    // passes per wave
  extern __shared__ __attribute__((aligned(16))) char smem[];  // carved by hand, see knn_scan_kernel
  char* tile0 = smem;                                                          // [2][KNN_TN * XSB]
  unsigned* q_mask = reinterpret_cast<unsigned*>(smem + 2 * KNN_TN * XSB);     // [PW_QB][PW_W][2]  bit = column of the slot's tile
  unsigned* q_occ = q_mask + PW_QB * PW_W * 2;                                 // [PW_QB]           bit = slot not empty
  float* tau_s = reinterpret_cast<float*>(q_occ + PW_QB);                      // [PW_QB]

  const int tid = threadIdx.x;
  const int lane = tid & 63, w = tid >> 6;
  const int half = lane >> 5, r32 = lane & 31;
  const int64_t qbase = (int64_t)blockIdx.x * PW_QB;
  const int d = a.d, k = a.k;
  const char* ptrain = reinterpret_cast<const char*>(a.packed_train);

  // ---- per-query state: tau = the largest entry of the list (a wave per query, coalesced) ----------------------------
  for (int r = 0; r < PW_QW; ++r) {
    const int qslot = w * PW_QW + r;
    const int64_t q = qbase + qslot;
    float t = -__builtin_inff();  // rows past the end never accept anything
    if (q < a.m) {
      for (int j = lane; j < k; j += 64) t = fmaxf(t, a.best_d[q * k + j]);
      t = wave_max(t);
    }
    if (lane == 0) tau_s[qslot] = t;
  }
  for (int t = tid; t < PW_QB * PW_W * 2; t += 256) q_mask[t] = 0u;
  q_occ[tid] = 0u;
  __syncthreads();
  // A operands: row block rb, lane (r32, half): pieces 2 J + half of query qbase + 64 w + 32 rb + r32, hi and lo parts
  u4x ahi[2][NQ], alo[2][NQ];
  float myqn[2];
  auto set_thr = [&](int rb, float tau) {  // (upper lanes) -thr of the row block's query into packed slot KP - 1
    unsigned hi, lo;
    neg_thr_split(myqn[rb], tau, hi, lo);
    ahi[rb][NQ - 1].w = (ahi[rb][NQ - 1].w & 0xFFFFu) | (hi << 16);
    alo[rb][NQ - 1].w = (alo[rb][NQ - 1].w & 0xFFFFu) | (lo << 16);
  };
#pragma unroll
  for (int rb = 0; rb < 2; ++rb) {
    const int row = w * PW_QW + rb * 32 + r32;
    const int64_t q = qbase + row;
    const char* prow = reinterpret_cast<const char*>(a.packed_queries) + (q < a.m ? q : 0) * (int64_t)RB;
#pragma unroll
    for (int j = 0; j < NQ; ++j) {
      ahi[rb][j] = *reinterpret_cast<const u4x*>(prow + 16 * (2 * j + half));
      alo[rb][j] = *reinterpret_cast<const u4x*>(prow + 2 * KP + 16 * (2 * j + half));
    }
    myqn[rb] = q < a.m ? a.query_sqn[q] : 0.f;
    if (half == 1) set_thr(rb, tau_s[row]);
  }

  // Staging through registers: slot sigma = 64 p + lane of a tile is row sigma / SPR, piece sigma % SPR (the padding slot
  // repeats the last piece); wave w takes passes w, w + 4, ..  Rows past n repeat row n - 1 and are masked by position.
  u4x stg[IPW];
  auto load_tile = [&](int64_t t0) {
#pragma unroll
    for (int it = 0; it < IPW; ++it) {
      const int p = min(w + 4 * it, SPR - 1);
      const int sigma = 64 * p + lane;
      const int row = sigma / SPR;
      const int c = min(sigma - row * SPR, SPR - 2);
      const int64_t grow = min(t0 + row, a.n - 1);
      stg[it] = *reinterpret_cast<const u4x*>(ptrain + grow * (int64_t)RB + c * 16);
    }
  };
  auto store_tile = [&](int buf) {
#pragma unroll
    for (int it = 0; it < IPW; ++it)
      if (w + 4 * it < SPR) *reinterpret_cast<u4x*>(tile0 + buf * KNN_TN * XSB + (w + 4 * it) * 1024 + lane * 16) = stg[it];
  };
  // staggered walk over the table (see knn_scan_kernel), two running indices (see knn_scan_bf16x3_kernel)
  const int64_t ntiles = (a.n - a.start + KNN_TN - 1) / KNN_TN;
  const int64_t tile_off = ((int64_t)blockIdx.x * 7919) % ntiles;
  auto tile_after = [&](int64_t t) { return t + 1 == ntiles ? (int64_t)0 : t + 1; };
  int64_t tcur = tile_off, tahead = tile_off;  // tile of step tj / the next tile to request
  load_tile(a.start + tahead * KNN_TN);
  tahead = tile_after(tahead);
  store_tile(0);
  int buf = 0;
  int wfill = 0;             // tiles in the window
  int64_t wfirst = tile_off;  // the tile of window slot 0
  for (int64_t tj = 0; tj < ntiles; ++tj, buf ^= 1, tcur = tile_after(tcur)) {
    const int64_t t0 = a.start + tcur * KNN_TN;
    __syncthreads();  // tile tj is in buffer `buf` (everyone's stores), and nobody still reads the other buffer
    const bool more = tj + 1 < ntiles;
    if (more) {
      load_tile(a.start + tahead * KNN_TN);
      tahead = tile_after(tahead);
    }
    const char* tl = tile0 + buf * KNN_TN * XSB;
    const int nvalid = (int)(a.n - t0 < (int64_t)KNN_TN ? a.n - t0 : (int64_t)KNN_TN);  // rows of this tile that exist
    // this tile's window slot of the lane's first query row, and that row's slot word
    unsigned* mslot = q_mask + ((w * PW_QW + 4 * half) * PW_W + wfill) * 2;
    unsigned* oslot = q_occ + w * PW_QW + 4 * half;
#pragma unroll
    for (int ct = 0; ct < KNN_TN / 32; ++ct) {
      const char* xrow = tl + (ct * 32 + r32) * XSB;
      u4x bhi[NQ], blo[NQ];
#pragma unroll
      for (int j = 0; j < NQ; ++j) {
        bhi[j] = *reinterpret_cast<const u4x*>(xrow + 16 * (2 * j + half));
        blo[j] = *reinterpret_cast<const u4x*>(xrow + 2 * KP + 16 * (2 * j + half));
      }
#pragma unroll
      for (int rb = 0; rb < 2; ++rb) {
        f16x acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < NQ; ++j)
          acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf8x, ahi[rb][j]), __builtin_bit_cast(bf8x, bhi[j]),
                                                        acc, 0, 0, 0);
#pragma unroll
        for (int j = 0; j < NQ; ++j)
          acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf8x, ahi[rb][j]), __builtin_bit_cast(bf8x, blo[j]),
                                                        acc, 0, 0, 0);
#pragma unroll
        for (int j = 0; j < NQ; ++j)
          acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf8x, alo[rb][j]), __builtin_bit_cast(bf8x, bhi[j]),
                                                        acc, 0, 0, 0);
        // survivors: any accumulator positive?  (as integers: v_max3_i32, see knn_scan_bf16x3_kernel)
        int mx = max(__float_as_int(acc[0]), __float_as_int(acc[1]));
#pragma unroll
        for (int v = 2; v < 16; v += 2) mx = max(mx, max(__float_as_int(acc[v]), __float_as_int(acc[v + 1])));
        if (mx > 0 && ct * 32 + r32 < nvalid) {
#pragma unroll
          for (int v = 0; v < 16; ++v) {
            if (acc[v] > 0.f) {  // query row rb 32 + tile_acc_row(v, half) of the wave: a constant offset from the lane's base
              const int qoff = rb * 32 + 8 * (v >> 2) + (v & 3);
              atomicOr(mslot + qoff * PW_W * 2 + ct, 1u << r32);
              atomicOr(oslot + qoff, 1u << wfill);
            }
          }
        }
      }
    }
    if (more) store_tile(buf ^ 1);  // (everyone passed this step's barrier: nobody reads that buffer any more)
    ++wfill;

    // ---- drain (wave-private state: no barrier) ------------------------------------------------------------------------
    // cadence in ROWS the lists have seen, as in knn_scan_bf16x3_kernel, never longer than the window
    {
      constexpr int64_t per_tile = MGP_KNN_CADENCE ? (int64_t)MGP_KNN_CADENCE * KNN_TN : 1;  // (0: every full window)
      const int64_t every = MGP_KNN_CADENCE ? (a.start + tj * KNN_TN) / per_tile : PW_W;  // in tiles
      if (wfill < PW_W && wfill < every && more) continue;
    }
    wave_lds_fence();
    const unsigned myocc = qbase + w * PW_QW + lane < a.m ? q_occ[w * PW_QW + lane] : 0u;  // lane = query of the wave
    unsigned long long pending = __ballot(myocc != 0u);
    if (pending) {
      float vnext[KNN_EPL];
      load_list(a.best_d, qbase + w * PW_QW + __builtin_ctzll(pending), k, lane, vnext);
      while (pending) {
        const int r = __builtin_ctzll(pending);
        pending &= pending - 1;
        const int qslot = w * PW_QW + r;
        const int64_t q = qbase + qslot;
        float v[KNN_EPL];
#pragma unroll
        for (int e = 0; e < KNN_EPL; ++e) v[e] = vnext[e];
        if (pending) load_list(a.best_d, qbase + w * PW_QW + __builtin_ctzll(pending), k, lane, vnext);
        unsigned slots = __shfl(myocc, r, 64);  // (wave-uniform)
        const int64_t self = a.self_idx ? a.self_idx[q] : -1;
        const float* qrow = a.queries + q * (int64_t)d;
        float lmax;
        int lpos;
        lane_max(v, lmax, lpos);
        float tau = wave_max(lmax);
        float* ld = a.best_d + q * (int64_t)k;
        int* li = a.best_i + q * (int64_t)k;
        while (slots) {
          const int s = __builtin_ctz(slots);
          slots &= slots - 1;
          const int64_t tile = wfirst + s < ntiles ? wfirst + s : wfirst + s - ntiles;
          const int64_t t0s = a.start + tile * KNN_TN;
          const int64_t row = t0s + lane;  // lane = column of the slot's tile
          const bool mine = ((q_mask[(qslot * PW_W + s) * 2 + half] >> r32) & 1u) && row != self && row < a.n;
          float cd = __builtin_inff();
          if (mine) {  // the exact distance: the arithmetic of knn_scan_bf16x3_kernel's drain
            const float* xrow = a.train + row * (int64_t)d;
            cd = 0.f;
            for (int c = 0; c < d; c += 4) {
              const f4x df = *reinterpret_cast<const f4x*>(qrow + c) - *reinterpret_cast<const f4x*>(xrow + c);
              cd += df.x * df.x + df.y * df.y + df.z * df.z + df.w * df.w;
            }
          }
          unsigned long long cand = __ballot(mine && cd < tau);
          while (cand) {
            const int c = __builtin_ctzll(cand);
            cand &= cand - 1;
            const float ccd = __shfl(cd, c, 64);
            if (!(ccd < tau)) continue;  // (tau has tightened since the ballot)
            // the first lane whose own maximum is the list's: it replaces that one entry, here and in global memory
            const unsigned long long at_max = __ballot(lmax == tau);
            if (lane == __builtin_ctzll(at_max)) {
#pragma unroll
              for (int e = 0; e < KNN_EPL; ++e)
                if (e == lpos) v[e] = ccd;
              ld[lpos * 64 + lane] = ccd;
              li[lpos * 64 + lane] = (int)(t0s + c);
              lane_max(v, lmax, lpos);
            }
            tau = wave_max(lmax);
          }
        }
        if (lane == 0) {
          tau_s[qslot] = tau;
          q_occ[qslot] = 0u;
        }
        if (lane < 2 * PW_W) q_mask[qslot * PW_W * 2 + lane] = 0u;
      }
      // only this wave's rows can have changed: make the writes visible to the wave, then the new -thr slots
      __builtin_amdgcn_s_waitcnt(0);
      wave_lds_fence();
      if (half == 1) {
#pragma unroll
        for (int rb = 0; rb < 2; ++rb) set_thr(rb, tau_s[w * PW_QW + rb * 32 + r32]);
      }
    }
    wfill = 0;
    wfirst = tile_after(tcur);
  }
}

template <int KP>
static int launch_knn_prefilter_wide_kp(const KnnPackedArgs& a, hipStream_t stream) {
  constexpr size_t lds = pw_lds_bytes(KP);
  static_assert(lds <= 64 * 1024, "no opt-in needed, and two workgroups per CU");
  const int64_t grid = (a.m + PW_QB - 1) / PW_QB;
  hipLaunchKernelGGL(knn_prefilter_wide_kernel<KP>, dim3((unsigned)grid), dim3(256), lds, stream, a);
  MGP_HIP_CHECK_LAUNCH();
  return MGP_OK;
}

int launch_knn_prefilter_wide(const KnnPackedArgs& a, hipStream_t stream) {
  if (a.k < 1 || a.k > KNN_WIDE_MAX_K || a.d < 4 || a.d % 4 != 0 || a.d > 64) return MGP_EUNSUPPORTED;
  const uintptr_t al = (uintptr_t)a.train | (uintptr_t)a.queries | (uintptr_t)a.packed_train | (uintptr_t)a.packed_queries;
  if (al % 16 != 0) return MGP_EUNSUPPORTED;
  if (a.n >= (int64_t)1 << 31) return MGP_EUNSUPPORTED;  // list indices are 32-bit
  // the IN lists must be whole: k rows below start, one more where a query's own row may be among them
  if ((int64_t)a.k + (a.self_idx ? 1 : 0) > a.start) return MGP_EUNSUPPORTED;
  if ((a.m + PW_QB - 1) / PW_QB >= (int64_t)1 << 31) return MGP_EUNSUPPORTED;
  switch ((a.d + 2 + 15) / 16 * 16) {  // features + the two threshold slots
    case 16: return launch_knn_prefilter_wide_kp<16>(a, stream);
    case 32: return launch_knn_prefilter_wide_kp<32>(a, stream);
    case 48: return launch_knn_prefilter_wide_kp<48>(a, stream);
    case 64: return launch_knn_prefilter_wide_kp<64>(a, stream);
    default: return launch_knn_prefilter_wide_kp<80>(a, stream);
  }
}

}  // namespace mgp
