// Exact k-NN for tables of 1 to 3 features: a per-query walk over the cells of a rectilinear grid, shell by shell,
// until the geometry of the walked block proves the list final.
//
// The table is stored cell by cell (muygpys_amd/neighbors.py: the index); the linear cell id runs with axis 0 fastest,
// so the cells c0 - r .. c0 + r of one grid row are ONE contiguous run of stored rows.  One wave serves one query; the
// four waves of a workgroup are independent (no barrier, no shared state, no workgroup waits on another, no atomics).
// The list, the pending slots, admission and merge are those of the cell scan (mgp_knn_list.h), and so is the step
// loop: per step every lane takes one row of the current run, 16 bytes, and measures it in the difference form, fp32;
// the rows of the next step are requested before the current ones are compared.
//
//   walk    shell r = 0, 1, 2 ... is every cell at Chebyshev cell distance exactly r from the query's cell that lies
//           inside the grid: a whole run for a grid row the shell opens (|j1 - c1| or |j2 - c2| equals r), the two end
//           cells c0 - r and c0 + r for a grid row that is already open.
//   merge   after the shell, so that tau is the k-th best distance (+inf while fewer than k rows are held).
//   bound   the block c_a - r .. c_a + r, clipped to the grid, is [l_a, h_a] per axis.  On the low side of axis a cells
//           remain if l_a > 0, and every row in them has x_a < E_a[l_a - 1] <= q_a; on the high side if
//           h_a < g_a - 1, and every row there has x_a >= E_a[h_a] > q_a.  t = q_a - E_a[l_a - 1] (E_a[h_a] - q_a) is
//           the distance to that face and B the smallest t of the sides with cells left.
//   stop    when no side has cells left (the block is the grid), or when tau < B^2 (1 - 2^-20) on every such side.
//           The inequality is strict: every row tied with the k-th has then been seen, and because ties are taken in
//           order of stored position (mgp_knn_list.h) the result is a function of the table alone.
//
// The slack.  An unvisited row x behind the low face of axis a has x_a < E <= q_a, so q_a - x_a > q_a - E >= 0 in exact
// arithmetic.  Its distance as this kernel measures it is dd = fl(fl(s0 + s1) + fl(s2 + s3)), s_c = fl(e_c^2),
// e_c = fl(q_c - x_c).  Counting roundings without looking at their direction: e_a carries one (2^-24 relative), its
// square two more and one of its own, the two additions one each; the threshold carries one in t, two in t^2 and one
// in the product: about 8 units of 2^-24 between "dd of an unvisited row" and "t^2 as computed" in the worst case.
// 1 - 2^-20 is 16 units.  Looking at the direction, none is needed: rounding is monotone, so e_a >= fl(q_a - E) = t
// bit for bit, fl(e_a^2) >= fl(t^2), and adding non-negative terms and rounding never goes below a term: dd >= fl(t^2)
// >= fl(fl(t^2) (1 - 2^-20)) > tau.  (The square is a plain product in both places -- fma(e, e, 0) rounds once, like the
// multiplication -- and flushing denormals is monotone too.)  A slack that is too large costs cells, never
// correctness.  A t that is not positive (a qcell that contradicts the query: the raw entry takes any) stops nothing:
// the bound holds for every qcell, and the result is exact whatever qcell says.
//
// The trip count of the shell loop is at most gmax = max(g0, g1, g2), a kernel argument: at r = gmax - 1 the block is
// the grid wherever the query's cell lies.  A non-finite coordinate (query, row or edge) makes its comparisons false:
// nothing stops early on it, nothing is admitted at a NaN distance, and the walk ends at the grid's edge.
// qcell is clamped to the grid and cell_start to [0, n]: no argument value indexes outside cell_start or the table.
//
// Resources (lib/kernel_resources.json; tests/test_knn_grid_resources.py compares this line with the report):
//   kernel                 VGPRs  SGPRs  waves/SIMD  spilled VGPRs  scratch
//   knn_grid_scan_kernel   24     96     8           0              0
//
// Reference: the exact branch of the reference's neighbour search with algorithm="kd_tree" / "ball_tree" (scikit-learn
// behind NN_Wrapper, src/MuyGPyS/neighbors.py:89-107), sub-quadratic at low d.
#include <cstdint>

#include "mgp_args.h"
#include "mgp_knn_list.h"

namespace mgp {

namespace {

constexpr int64_t kGridMaxCells = (int64_t)1 << 24;

struct GridScanArgs {
  const float* table;
  const int64_t* cell_start;
  const float* edges;
  const float* queries;
  const int* qcell;
  const int64_t* self_pos;
  float* best_d;
  int* best_i;
  int* shells;
  int64_t n, m;
  int g0, g1, g2, gmax, k;
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__global__ __launch_bounds__(kCellWaves * 64) void knn_grid_scan_kernel(const GridScanArgs a) {
  __shared__ float s_dist[kCellWaves][kCellSlots];
  __shared__ int s_pos[kCellWaves][kCellSlots];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t q = (int64_t)blockIdx.x * kCellWaves + wave;
  if (q >= a.m) return;
  WaveList list(s_dist[wave], s_pos[wave], lane, a.k);

  // the query row and its cell: wave-uniform addresses -> scalar registers
  const float4 qv = *reinterpret_cast<const float4*>(a.queries + q * 4);
  const int64_t self = a.self_pos ? a.self_pos[q] : (int64_t)-1;
  const int g0 = a.g0, g1 = a.g1, g2 = a.g2;
  const int c0 = clampi(a.qcell[q * 3 + 0], 0, g0 - 1);
  const int c1 = clampi(a.qcell[q * 3 + 1], 0, g1 - 1);
  const int c2 = clampi(a.qcell[q * 3 + 2], 0, g2 - 1);
  const float* E0 = a.edges;  // (g - 1 interior edges per axis; none is read on an axis of one cell)
  const float* E1 = E0 + (g0 - 1);
  const float* E2 = E1 + (g1 - 1);

  int sh = 0;                              // the shell
  int l0, h0, l1, h1, l2, h2;              // the block c_a - sh .. c_a + sh, clipped to the grid
  int j1 = 0, j2 = 0, piece = 0;           // the grid row the next run comes from, and which of its pieces
  int64_t r = 0, e = 0;                    // the rows of the current run not yet requested
  // the steps of a shell: (first row, end of its run), run after run
  auto next_step = [&]() -> bool {
    while (r >= e) {
      if (j2 > h2) return false;
      const int d1 = j1 > c1 ? j1 - c1 : c1 - j1, d2 = j2 > c2 ? j2 - c2 : c2 - j2;
      const bool opens = (d1 > d2 ? d1 : d2) == sh;  // the shell opens this grid row: the whole run; else its end cells
      int lo = 0, hi = -1;
      if (opens) {
        lo = l0;
        hi = h0;
      } else if (piece == 0) {
        if (c0 - sh >= 0) lo = hi = c0 - sh;
      } else {
        if (c0 + sh <= g0 - 1) lo = hi = c0 + sh;
      }
      const int row = (j2 * g1 + j1) * g0;  // (< g0 g1 g2 <= 2^24)
      if (!opens && piece == 0) {
        piece = 1;
      } else {
        piece = 0;
        if (++j1 > h1) {
          j1 = l1;
          ++j2;
        }
      }
      if (lo <= hi) {  // (0 <= lo, hi <= g0 - 1: the last index is row + g0 <= g0 g1 g2)
        r = a.cell_start[row + lo];
        e = a.cell_start[row + hi + 1];
        if (r < 0) r = 0;
        if (e > a.n) e = a.n;
      }
    }
    return true;
  };
  auto load_rows = [&](float4& x, int64_t& row) {
    row = r + lane;
    const int64_t at = row < e ? row : e - 1;  // (lanes past the end of the run read its last row and drop it)
    x = *reinterpret_cast<const float4*>(a.table + at * 4);
  };

  while (true) {
    l0 = c0 - sh < 0 ? 0 : c0 - sh;
    h0 = c0 + sh > g0 - 1 ? g0 - 1 : c0 + sh;
    l1 = c1 - sh < 0 ? 0 : c1 - sh;
    h1 = c1 + sh > g1 - 1 ? g1 - 1 : c1 + sh;
    l2 = c2 - sh < 0 ? 0 : c2 - sh;
    h2 = c2 + sh > g2 - 1 ? g2 - 1 : c2 + sh;
    j1 = l1;
    j2 = l2;
    piece = 0;
    r = e = 0;

    float4 cur, nxt;
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
      const float e0 = qv.x - cur.x, e1 = qv.y - cur.y, e2 = qv.z - cur.z, e3 = qv.w - cur.w;
      const float s0 = __builtin_fmaf(e0, e0, 0.f), s1 = __builtin_fmaf(e1, e1, 0.f);
      const float s2 = __builtin_fmaf(e2, e2, 0.f), s3 = __builtin_fmaf(e3, e3, 0.f);
      const float dd = (s0 + s1) + (s2 + s3);
      list.admit(cur_row < cur_end && cur_row != self && dd <= list.tau, dd, cur_row);
      have = have_next;
      if (have_next) {
        cur = nxt;
        cur_row = nxt_row;
        cur_end = nxt_end;
      }
    }
    if (list.npend > 0) list.merge();

    // the faces behind which cells remain; done: tau is below the squared distance to every one of them
    constexpr float kSlack = 1.f - 0x1p-20f;
    const float tau = list.tau;
    bool open = false, done = true;
    auto face = [&](bool cells_left, float t) {
      if (cells_left) {
        open = true;
        done = done && t > 0.f && tau < (t * t) * kSlack;
      }
    };
    face(l0 > 0, qv.x - (l0 > 0 ? E0[l0 - 1] : 0.f));
    face(h0 < g0 - 1, (h0 < g0 - 1 ? E0[h0] : 0.f) - qv.x);
    face(l1 > 0, qv.y - (l1 > 0 ? E1[l1 - 1] : 0.f));
    face(h1 < g1 - 1, (h1 < g1 - 1 ? E1[h1] : 0.f) - qv.y);
    face(l2 > 0, qv.z - (l2 > 0 ? E2[l2 - 1] : 0.f));
    face(h2 < g2 - 1, (h2 < g2 - 1 ? E2[h2] : 0.f) - qv.z);
    if (!open || done || sh + 1 >= a.gmax) break;
    ++sh;
  }

  list.store(a.best_d, a.best_i, q);
  if (lane == 0) a.shells[q] = sh;
}

}  // namespace

}  // namespace mgp

extern "C" int mgp_knn_grid_scan(const float* table, int64_t n, const int64_t* cell_start, int g0, int g1, int g2,
                                 const float* edges, const float* queries, int64_t m, const int32_t* qcell,
                                 const int64_t* self_pos, int k, float* best_d, int32_t* best_i, int32_t* shells,
                                 void* stream) {
  using namespace mgp;
  if (n < 0 || m < 0 || k < 1 || g0 < 1 || g1 < 1 || g2 < 1) return MGP_EINVAL;
  if (m == 0) return MGP_OK;
  if (!table || !cell_start || !queries || !qcell || !best_d || !best_i || !shells) return MGP_EINVAL;
  if (!edges && (g0 > 1 || g1 > 1 || g2 > 1)) return MGP_EINVAL;
  int64_t cells = g0;  // (each factor < 2^31 and the running product <= 2^24 before the next: no overflow)
  if (cells <= kGridMaxCells) cells *= g1;
  if (cells <= kGridMaxCells) cells *= g2;
  if (k > kCellList || n >= ((int64_t)1 << 31) || cells > kGridMaxCells) return MGP_EUNSUPPORTED;
  if (((uintptr_t)table | (uintptr_t)queries) % 16 != 0) return MGP_EUNSUPPORTED;
  if ((m + kCellWaves - 1) / kCellWaves >= ((int64_t)1 << 31)) return MGP_EUNSUPPORTED;
  const int gmax = g0 > g1 ? (g0 > g2 ? g0 : g2) : (g1 > g2 ? g1 : g2);
  const GridScanArgs a{table, cell_start, edges, queries, qcell, self_pos, best_d, best_i, shells, n, m, g0, g1, g2, gmax, k};
  const unsigned grid = (unsigned)((m + kCellWaves - 1) / kCellWaves);
  hipLaunchKernelGGL(knn_grid_scan_kernel, dim3(grid), dim3(kCellWaves * 64), 0, static_cast<hipStream_t>(stream), a);
  MGP_HIP_CHECK_LAUNCH();
  return MGP_OK;
}
