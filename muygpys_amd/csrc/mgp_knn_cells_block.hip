// Approximate k-NN over the inverted-cell (IVF) index: the BLOCK scan of the probed cells, on the matrix cores.
//
// mgp_knn_cells.hip serves one query per wave on the vector unit.  This kernel is built on the tile of the exact scan
// (knn_scan_kernel, mgp_knn.hip; the shared pieces are in mgp_knn_tile.h) and streams a different thing through it: not
// the whole table, but the union of the cells that the workgroup's queries probe.
//
//   work split  a workgroup of four waves owns 128 consecutive queries, 32 per wave; their feature rows are the resident
//               MFMA A operand (v_mfma_f32_32x32x2_f32, fp32 in / fp32 accumulate).  The caller orders the queries by
//               nearest cell, so a block's queries share most of their probes.  The accumulator starts at -|x|^2/2 and
//               is compared against (|q|^2 - tau)/2: ONE compare per pair.
//   union       a bitmap of nlist <= 4 096 bits in LDS; every thread ORs the cells of its own query into it (LDS atomics;
//               the cell a query's list was seeded from, skip_cell, is left out).  The workgroup visits the set bits in
//               ascending order -- the table is stored cell by cell, so this is an ascending walk through memory.
//   staging     each cell in double-buffered tiles of 64 rows (global_load_lds_dwordx4, row stride XS = DP + 4 floats),
//               the next tile -- of this cell or the next one -- in flight under the MFMAs.  |x|^2 of the tile's rows
//               comes from table_sqn by one global_load_lds_dword per tile; a lane whose row lies at or past the cell's
//               end reads table_sqn[n] = +inf instead, so that no compare passes for it.  Empty cells stage nothing.
//   membership  a pair counts only if the cell is one of the query's probes.  Lane l < 32 of wave w keeps a cursor into
//               the (ascending) probe row of query 32 w + l -- the row stays in global memory / L1, nprobe may be nlist --
//               and advances it as the cells go by.  At the first tile of a cell it writes the query's effective bound to
//               LDS: tau if the cell is probed and is not skip_cell[q], otherwise -inf (a threshold of +inf: no pair
//               passes).  These slots are wave-private, so no workgroup barrier is spent on them.  A wave none of whose
//               queries probes the cell skips the cell's MFMAs (wave-uniform test) and only meets the tile barriers.
//   selection   the exact scan's: pairs that pass go to per-query queues in LDS (16 entries); after each tile the owning
//               wave drains them into the query's k-best list (one element per lane, replace the maximum) and tightens
//               tau.  The element replaced is the largest by (distance, position) and a candidate enters only if it is
//               smaller in that order, so a list does not depend on the order its candidates arrived in.  The self-match
//               self_pos[q] is dropped.
//   overflow    a queue that took more than 16 pairs in one tile: if the list was not yet full (tau = +inf: the seed
//               cell held fewer than k rows, every pair passes) the query is marked in overflow[] and the caller
//               recomputes it with the per-query scan.  If the list was full, the owning wave measures the tile's 64 rows
//               against that query directly (one row per lane, vector unit) and merges them: nothing is lost, nothing is
//               flagged.  Either way the decision depends on the query's own state alone.
//
// No global atomics, no workgroup waits on another, every write to global memory is a plain vector store.
//
// Distances in the lists are the Gram form |q|^2 + |x|^2 - 2 q.x; mgp_knn_finish_f32 re-measures and sorts them.
//
// Measured (tools/ivfbench.py --cell-scan block -> profiles/knn_ivf_block_bench.json): against the
// per-query scan 0.34 x (d = 8, 1 M rows, 4 probes) to 7.2 x (d = 40 mixture, 64 probes); it wins where the union of a
// block's cells is small next to 128 nprobe, i.e. at many probes and on clustered tables, and loses at few probes.
//
// Resources (lib/kernel_resources.json, gfx950; no instantiation spills or uses scratch; LDS is dynamic,
// 512 DP + 20 992 bytes: two tiles, their norms, the queues, three floats per query, the bitmap):
//   DP      VGPRs  SGPRs  LDS bytes  waves / SIMD
//    8      126    101    25 088     4
//   16      138    105    29 184     3
//   24      136    105    33 280     3
//   32      140    105    37 376     3
//   40      144    105    41 472     3
//   48      148    105    45 568     3
//   56      152    105    49 664     3
//   64      156    105    53 760     3
#include <cstdint>

#include "mgp_args.h"
#include "mgp_knn_list.h"
#include "mgp_knn_tile.h"

namespace mgp {

namespace {

constexpr int CB_WORDS = 128;  // bitmap words: nlist <= 4 096

struct CellBlockArgs {
  const float* table;
  const float* table_sqn;
  const int64_t* cell_start;
  const float* queries;
  const float* query_sqn;
  const int* probes;
  const int64_t* skip_cell;
  const int64_t* self_pos;
  float* best_d;
  int* best_i;
  int* overflow;
  int64_t n, m;
  int nlist, nprobe, k, d;
};

struct CellTile {
  int64_t t0, end;  // first row of the tile, end of its cell
  int cell;
  bool fresh;       // the cell's first tile
};

template <int DP>
__global__ __launch_bounds__(256) void knn_cells_block_kernel(const CellBlockArgs a) {
  constexpr int XS = DP + 4;  // LDS row stride: an odd number of 16-byte slots
  constexpr int HD = DP / 2;  // features per lane half
  // one extern array carved by hand, see knn_scan_kernel
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* tile0 = reinterpret_cast<float*>(smem);                          // [2][KNN_TN * XS]
  float* xn0 = tile0 + 2 * KNN_TN * XS;                                   // [2][KNN_TN]
  float* q_d = xn0 + 2 * KNN_TN;                                          // [KNN_QB * KNN_CAP]
  int* q_i = reinterpret_cast<int*>(q_d + KNN_QB * KNN_CAP);              // [KNN_QB * KNN_CAP]
  int* q_cnt = q_i + KNN_QB * KNN_CAP;                                    // [KNN_QB]
  float* tau_s = reinterpret_cast<float*>(q_cnt + KNN_QB);                // [KNN_QB] the k-th best of every query
  float* eff_s = tau_s + KNN_QB;                                          // [KNN_QB] ... or -inf where the cell is not probed
  unsigned* bitmap = reinterpret_cast<unsigned*>(eff_s + KNN_QB);         // [CB_WORDS] the union of the probed cells

  const int tid = threadIdx.x;
  const int lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int half = lane >> 5, r32 = lane & 31;
  const int64_t qbase = (int64_t)blockIdx.x * KNN_QB;
  const int d = a.d, k = a.k;
  const float inf = __builtin_inff();

  // ---- per-query state, the union of the probed cells ------------------------------------------------------------
  if (tid < KNN_QB) {
    const int64_t q = qbase + tid;
    float t = -inf;  // rows past the end never accept anything
    if (q < a.m) {
      t = a.best_d[q * k];
      for (int j = 1; j < k; ++j) t = fmaxf(t, a.best_d[q * k + j]);
      a.overflow[q] = 0;
    }
    tau_s[tid] = t;
    eff_s[tid] = -inf;
    q_cnt[tid] = 0;
    bitmap[tid] = 0u;
  }
  __syncthreads();
  {
    const int slot = tid & (KNN_QB - 1);
    const int64_t q = qbase + slot;
    if (q < a.m) {
      const int* pr = a.probes + q * (int64_t)a.nprobe;
      const int64_t skip = a.skip_cell ? a.skip_cell[q] : (int64_t)-1;
      for (int j = tid >> 7; j < a.nprobe; j += 2) {
        const int c = pr[j];
        if (c >= 0 && c < a.nlist && c != skip) atomicOr(&bitmap[c >> 5], 1u << (c & 31));
      }
    }
  }
  // A operand: lane (r32, half) holds features [half*HD, half*HD + HD) of query qbase + 32 w + r32
  float aq[HD];
  {
    const int64_t q = qbase + w * KNN_QW + r32;
    const float* qrow = a.queries + (q < a.m ? q : 0) * (int64_t)d;
#pragma unroll
    for (int j = 0; j < HD / 4; ++j) {
      const int c = half * HD + 4 * j;
      f4x v = {0.f, 0.f, 0.f, 0.f};
      if (c < d) v = *reinterpret_cast<const f4x*>(qrow + c);
      aq[4 * j] = v.x, aq[4 * j + 1] = v.y, aq[4 * j + 2] = v.z, aq[4 * j + 3] = v.w;
    }
  }
  float qn[16], thr[16];
#pragma unroll
  for (int v = 0; v < 16; ++v) {
    const int64_t q = qbase + w * KNN_QW + 8 * (v >> 2) + 4 * half + (v & 3);
    qn[v] = q < a.m ? a.query_sqn[q] : 0.f;
    thr[v] = inf;
  }
  auto load_thr = [&]() {
#pragma unroll
    for (int v = 0; v < 16; ++v) thr[v] = 0.5f * (qn[v] - eff_s[w * KNN_QW + 8 * (v >> 2) + 4 * half + (v & 3)]);
  };
  // the membership cursor of query 32 w + lane (lanes 0 .. 31): pv = probes[q][pc], the first one not yet passed
  const int myslot = w * KNN_QW + r32;
  const int64_t myq = qbase + myslot;
  const bool owner = lane < KNN_QW && myq < a.m;
  const int* mypr = a.probes + (owner ? myq : 0) * (int64_t)a.nprobe;
  const int64_t myskip = owner && a.skip_cell ? a.skip_cell[myq] : (int64_t)-1;
  int pc = 0;
  int pv = owner ? mypr[0] : 0x7FFFFFFF;
  bool member = false;
  __syncthreads();  // the bitmap is complete

  // ---- the tiles of the walk: cell after cell of the union, 64 rows at a time (workgroup-uniform) -------------------
  const int nwords = (a.nlist + 31) >> 5;
  int wi = 0;
  unsigned bits = __builtin_amdgcn_readfirstlane(bitmap[0]);
  int cell = -1;
  int64_t r = 0, e = 0;
  auto next_tile = [&](CellTile& t) -> bool {
    bool fresh = false;
    while (r >= e) {
      while (bits == 0u) {
        if (++wi >= nwords) return false;
        bits = __builtin_amdgcn_readfirstlane(bitmap[wi]);
      }
      cell = wi * 32 + __builtin_ctz(bits);
      bits &= bits - 1u;
      r = a.cell_start[cell];
      e = a.cell_start[cell + 1];
      if (r < 0) r = 0;
      if (e > a.n) e = a.n;
      fresh = true;
    }
    t.t0 = r, t.end = e, t.cell = cell, t.fresh = fresh;
    r += KNN_TN;
    return true;
  };
  // staging (tile_stage_rows): rows past the cell's end are read as they are (rows of the next cell; past n, row n - 1)
  // and masked by their norm alone
  const int dslots = d / 4;
  auto issue_tile = [&](int buf, const CellTile& t) {
    tile_stage_rows<DP>(tile0 + buf * KNN_TN * XS, a.table, a.n, d, dslots, t.t0, w, lane);
    if (w == 3) {
      const int64_t row = t.t0 + lane;
      lds_dma4(a.table_sqn + (row < t.end ? row : a.n), lds_offset(xn0 + buf * KNN_TN));
    }
  };

  CellTile cur, nxt;
  bool have = next_tile(cur);
  if (have) issue_tile(0, cur);
  int buf = 0;
  bool active = false;  // (wave-uniform) one of this wave's queries probes the current cell
  while (have) {
    const bool have_next = next_tile(nxt);
    __builtin_amdgcn_s_waitcnt(0);  // this wave's share of tile `buf` has landed
    __syncthreads();                // ... everyone's has, and nobody still reads the other buffer
    if (have_next) issue_tile(buf ^ 1, nxt);
    const float* tl = tile0 + buf * KNN_TN * XS;
    const float* xnt = xn0 + buf * KNN_TN;
    const int64_t t0 = cur.t0;

    if (cur.fresh) {
      if (lane < KNN_QW) {
        while (pv < cur.cell) {
          ++pc;
          pv = pc < a.nprobe ? mypr[pc] : 0x7FFFFFFF;
        }
        member = owner && pv == cur.cell && (int64_t)cur.cell != myskip;
        eff_s[myslot] = member ? tau_s[myslot] : -inf;
      }
      wave_lds_fence();
      active = __any(member);
      if (active) load_thr();
    }
    if (active) {
      f16x acc2[KNN_TN / 32];
#pragma unroll
      for (int ct = 0; ct < KNN_TN / 32; ++ct) {
        const int col = ct * 32 + r32;
        const float* xrow = tl + col * XS + half * HD;
        float bx[HD];
#pragma unroll
        for (int j = 0; j < HD / 4; ++j) {
          const f4x v = *reinterpret_cast<const f4x*>(xrow + 4 * j);
          bx[4 * j] = v.x, bx[4 * j + 1] = v.y, bx[4 * j + 2] = v.z, bx[4 * j + 3] = v.w;
        }
        const float c0 = -0.5f * xnt[col];
        f16x acc = {c0, c0, c0, c0, c0, c0, c0, c0, c0, c0, c0, c0, c0, c0, c0, c0};
#pragma unroll
        for (int t = 0; t < HD; ++t) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(aq[t], bx[t], acc, 0, 0, 0);
        acc2[ct] = acc;
      }
#pragma unroll
      for (int ct = 0; ct < KNN_TN / 32; ++ct) {
        const int col = ct * 32 + r32;
        const f16x acc = acc2[ct];
        bool any = false;
#pragma unroll
        for (int v = 0; v < 16; ++v) any = any || acc[v] > thr[v];
        if (any) {
#pragma unroll
          for (int v = 0; v < 16; ++v) {
            if (acc[v] > thr[v]) {
              const int qslot = w * KNN_QW + 8 * (v >> 2) + 4 * half + (v & 3);
              const int pos = atomicAdd(&q_cnt[qslot], 1);
              if (pos < KNN_CAP) {
                q_d[qslot * KNN_CAP + pos] = qn[v] - 2.0f * acc[v];
                q_i[qslot * KNN_CAP + pos] = (int)(t0 + col);
              }
            }
          }
        }
      }
      wave_lds_fence();

      // ---- drain this wave's queues into the k-best lists (wave-private state: no barrier) ----------------------
      const int mycnt = lane < KNN_QW ? q_cnt[myslot] : 0;
      unsigned long long pending = __ballot(mycnt > 0);
      const bool drained = pending != 0ull;
      while (pending) {
        const int qr = __builtin_ctzll(pending);
        pending &= pending - 1;
        const int qslot = w * KNN_QW + qr;
        const int64_t q = qbase + qslot;  // (< m: the other slots are no members of any cell)
        int cnt = q_cnt[qslot];
        const int self = a.self_pos ? (int)a.self_pos[q] : -1;
        float bd = lane < k ? a.best_d[q * k + lane] : -inf;
        int bi = lane < k ? a.best_i[q * k + lane] : -1;
        float tau = wave_max(bd);
        // (cd, ci) replaces the list's largest element by (distance, position) if it is smaller in that order
        auto insert = [&](float cd, int ci) {
          if (ci == self || !(cd <= tau)) return;
          const unsigned long long at_max = __ballot(bd == tau);
          int at = __builtin_ctzll(at_max);
          if (!(cd < tau) || (at_max & (at_max - 1))) {
            const int pm = wave_max(bd == tau ? bi : (int)0x80000000);
            if (!(cd < tau) && ci > pm) return;
            at = __builtin_ctzll(__ballot(bd == tau && bi == pm));
          }
          if (lane == at) bd = cd, bi = ci;
          tau = wave_max(bd);
        };
        if (cnt > KNN_CAP && tau < inf) {
          // a full list and a queue that lost pairs: the tile's 64 rows against this query, one row per lane
          const float* qrow = a.queries + q * (int64_t)d;
          const float* xrow = tl + lane * XS;
          float s = -0.5f * xnt[lane];
          for (int c = 0; c < d; c += 4) {
            const f4x qv = *reinterpret_cast<const f4x*>(qrow + c);
            const f4x xv = *reinterpret_cast<const f4x*>(xrow + c);
            s = __builtin_fmaf(qv.x, xv.x, s);
            s = __builtin_fmaf(qv.y, xv.y, s);
            s = __builtin_fmaf(qv.z, xv.z, s);
            s = __builtin_fmaf(qv.w, xv.w, s);
          }
          const float mine = a.query_sqn[q] - 2.0f * s;  // (+inf at and past the cell's end)
          unsigned long long todo = __ballot(mine <= tau);
          while (todo) {
            const int l = __builtin_ctzll(todo);
            todo &= todo - 1;
            insert(__shfl(mine, l, 64), (int)(t0 + l));
          }
        } else {
          if (cnt > KNN_CAP) {
            if (lane == 0) a.overflow[q] = 1;
            cnt = KNN_CAP;
          }
          for (int c = 0; c < cnt; ++c) insert(q_d[qslot * KNN_CAP + c], q_i[qslot * KNN_CAP + c]);
        }
        if (lane < k) {
          a.best_d[q * k + lane] = bd;
          a.best_i[q * k + lane] = bi;
        }
        if (lane == 0) {
          tau_s[qslot] = tau;
          q_cnt[qslot] = 0;
        }
      }
      if (drained) {  // (wave-uniform) only this wave's slots have changed
        wave_lds_fence();
        if (lane < KNN_QW && member) eff_s[myslot] = tau_s[myslot];
        wave_lds_fence();
        load_thr();
      }
    }
    have = have_next;
    cur = nxt;
    buf ^= 1;
  }
}

template <int DP>
int launch_cells_block(const CellBlockArgs& a, hipStream_t s) {
  const unsigned grid = (unsigned)((a.m + KNN_QB - 1) / KNN_QB);
  const size_t lds = (2 * KNN_TN * (DP + 4) + 2 * KNN_TN + 2 * KNN_QB * KNN_CAP + 3 * KNN_QB + CB_WORDS) * sizeof(float);
  hipLaunchKernelGGL(knn_cells_block_kernel<DP>, dim3(grid), dim3(256), lds, s, a);
  MGP_HIP_CHECK_LAUNCH();
  return MGP_OK;
}

}  // namespace

}  // namespace mgp

extern "C" int mgp_knn_cells_scan_block(const float* table, const float* table_sqn, int64_t n, int d,
                                        const int64_t* cell_start, int nlist, const float* queries,
                                        const float* query_sqn, int64_t m, const int32_t* probes, int nprobe,
                                        const int64_t* skip_cell, const int64_t* self_pos, int k, float* best_d,
                                        int32_t* best_i, int32_t* overflow, void* stream) {
  using namespace mgp;
  if (n < 0 || m < 0 || d < 1 || k < 1 || nlist < 1 || nprobe < 1 || nprobe > nlist) return MGP_EINVAL;
  if (d % 4 != 0 || d > 64 || k > 64 || nlist > 32 * CB_WORDS || n >= ((int64_t)1 << 31) ||
      (m + KNN_QB - 1) / KNN_QB >= ((int64_t)1 << 31))
    return MGP_EUNSUPPORTED;
  if (m == 0) return MGP_OK;
  if (!table || !table_sqn || !cell_start || !queries || !query_sqn || !probes || !best_d || !best_i || !overflow)
    return MGP_EINVAL;
  if (((uintptr_t)table | (uintptr_t)queries) % 16 != 0) return MGP_EUNSUPPORTED;
  const CellBlockArgs a{table, table_sqn, cell_start, queries, query_sqn, probes, skip_cell, self_pos,
                        best_d, best_i, overflow, n, m, nlist, nprobe, k, d};
  hipStream_t s = static_cast<hipStream_t>(stream);
  switch ((d + 7) / 8 * 8) {
    case 8: return launch_cells_block<8>(a, s);
    case 16: return launch_cells_block<16>(a, s);
    case 24: return launch_cells_block<24>(a, s);
    case 32: return launch_cells_block<32>(a, s);
    case 40: return launch_cells_block<40>(a, s);
    case 48: return launch_cells_block<48>(a, s);
    case 56: return launch_cells_block<56>(a, s);
    case 64: return launch_cells_block<64>(a, s);
  }
  return MGP_EUNSUPPORTED;
}
