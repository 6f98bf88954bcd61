// The slab of a local system beyond LDS and its blocked factorisation, shared by the forward kernels (mgp_large.hip)
// and the backward kernels on the slab (mgp_backward_large.h).  (The pair decoder of the triangle: mgp_assemble.h.)
//
// Slab: the lower trapezoid of the augmented system of mgp_lds_factor.h, row by row.  Row i < k holds its columns up
// to the end of its 32-column block (32 (i / 32 + 1) elements), the trailing rows hold KP = 32 ceil(k / 32) each; every
// row starts on a 128-byte boundary.  What lies right of the diagonal inside a diagonal block is never initialised
// and never reaches a result (see factor_augmented_slab).  The factorisation itself is described in mgp_large.hip.
#pragma once

#include "mgp_args.h"
#include "mgp_launch.h"
#include "mgp_lds_factor.h"
#include "mgp_wave_common.h"

namespace mgp {

constexpr int LNB = 32;  // panel width = side of a diagonal block

__host__ __device__ inline int large_kp(int k) { return (k + LNB - 1) / LNB * LNB; }
// element offset of row i of the slab of a system with k elimination columns
__host__ __device__ inline int large_row_off(int i, int k) {
  const int t = i < k ? i : k;
  const int q = t / LNB, r = t - q * LNB;
  const int tri = LNB * LNB * (q * (q + 1) / 2) + r * LNB * (q + 1);
  return i < k ? tri : tri + (i - k) * large_kp(k);
}
__host__ __device__ inline int large_slab_elems(int k, int R) { return large_row_off(k + 1 + R, k); }
// row stride of the LDS copy of a diagonal block: 16-byte aligned rows
template <typename T>
__host__ __device__ constexpr int large_lp() { return LNB + 16 / (int)sizeof(T); }

// launch rules of every kernel on a slab (the rest: mgp_launch.h): the cap of a recommended workspace, one workgroup per
// CU (104 - 217 registers at 512 threads), 256 threads up to 128 rows and 512 above
static const int64_t kMaxWorkspace = 512LL << 20;
static const int kMaxPerCu = 1;
static inline int slab_block_threads(int rows) { return rows <= 128 ? 256 : 512; }
// the slabs worth recommending for b systems: one per workgroup of a full grid
static inline int64_t slab_count(int64_t b) { return capacity_grid(b < 1 ? 1 : b, 0, Capacity{kMaxPerCu}); }

template <typename T>
struct SlabRows {
  T* S;
  int k;
  __device__ __forceinline__ T* operator()(int i) const { return S + large_row_off(i, k); }
};

// (lane_value -- the value lane `src`, a compile-time constant after unrolling, holds, as a wave-uniform scalar --
// is the one of mgp_wave_common.h, which the general-smoothness front end brings in anyway)

// step 1 of a panel, fp32: 32-row tiles on v_mfma_f32_32x32x2_f32.  Lane l feeds row (l & 31) of either operand; the
// instruction contracts over two columns per issue and the order of the columns is free as long as both operands
// agree, so lane half h = l >> 5 takes columns [c0 + 8 h, c0 + 8 h + 8) of a 16-column step as two 16-byte loads and
// issue e of the step contracts columns {c0 + e, c0 + 8 + e}: a fixed order, the same for every tile.
__device__ __forceinline__ void panel_update(SlabRows<float> row, int j0, int rows, int tid, int NT) {
  typedef float f4 __attribute__((ext_vector_type(4)));
  typedef float f16 __attribute__((ext_vector_type(16)));
  const int lane = tid & 63, wave = tid >> 6, nw = NT >> 6;
  const int m = lane & 31, h = lane >> 5;
  const int ntiles = (rows - j0 + 31) / 32;
  const float* pb = row(min(j0 + m, rows - 1)) + h * 8;  // (rows past the system: any valid row, results dropped)
  for (int t = wave; t < ntiles; t += nw) {
    const int i0 = j0 + 32 * t;
    const float* pa = row(min(i0 + m, rows - 1)) + h * 8;
    f16 acc = f16(0);
    f4 a0 = *reinterpret_cast<const f4*>(pa), a1 = *reinterpret_cast<const f4*>(pa + 4);
    f4 b0 = *reinterpret_cast<const f4*>(pb), b1 = *reinterpret_cast<const f4*>(pb + 4);
    for (int c0 = 0; c0 < j0; c0 += 16) {
      const f4 x0 = a0, x1 = a1, y0 = b0, y1 = b1;
      if (c0 + 16 < j0) {  // the next step's operands are in flight while this one is on the matrix pipe
        a0 = *reinterpret_cast<const f4*>(pa + c0 + 16), a1 = *reinterpret_cast<const f4*>(pa + c0 + 20);
        b0 = *reinterpret_cast<const f4*>(pb + c0 + 16), b1 = *reinterpret_cast<const f4*>(pb + c0 + 20);
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(x0[e], y0[e], acc, 0, 0, 0);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(x1[e], y1[e], acc, 0, 0, 0);
    }
    // accumulator g of lane l: row 8 (g / 4) + 4 (l >> 5) + g % 4, column l & 31
#pragma unroll
    for (int g = 0; g < 16; ++g) {
      const int i = i0 + 8 * (g / 4) + 4 * h + (g & 3);
      if (i < rows) row(i)[j0 + m] -= acc[g];
    }
  }
}

// ... fp64: 16-row tiles against the panel's two 16-column halves on v_mfma_f64_16x16x4_f64 (four columns per issue:
// lane quarter h = l >> 4 takes columns [c0 + 4 h, c0 + 4 h + 4) of a 16-column step)
__device__ __forceinline__ void panel_update(SlabRows<double> row, int j0, int rows, int tid, int NT) {
  typedef double d2 __attribute__((ext_vector_type(2)));
  typedef double d4 __attribute__((ext_vector_type(4)));
  const int lane = tid & 63, wave = tid >> 6, nw = NT >> 6;
  const int m = lane & 15, h = lane >> 4;
  const int ntiles = (rows - j0 + 15) / 16;
  const double* pb = row(min(j0 + m, rows - 1)) + h * 4;
  const double* pc = row(min(j0 + 16 + m, rows - 1)) + h * 4;
  for (int t = wave; t < ntiles; t += nw) {
    const int i0 = j0 + 16 * t;
    const double* pa = row(min(i0 + m, rows - 1)) + h * 4;
    d4 acc0 = d4(0), acc1 = d4(0);
    d2 a0 = *reinterpret_cast<const d2*>(pa), a1 = *reinterpret_cast<const d2*>(pa + 2);
    d2 b0 = *reinterpret_cast<const d2*>(pb), b1 = *reinterpret_cast<const d2*>(pb + 2);
    d2 c0v = *reinterpret_cast<const d2*>(pc), c1v = *reinterpret_cast<const d2*>(pc + 2);
    for (int c0 = 0; c0 < j0; c0 += 16) {
      const d2 x0 = a0, x1 = a1, y0 = b0, y1 = b1, z0 = c0v, z1 = c1v;
      if (c0 + 16 < j0) {
        a0 = *reinterpret_cast<const d2*>(pa + c0 + 16), a1 = *reinterpret_cast<const d2*>(pa + c0 + 18);
        b0 = *reinterpret_cast<const d2*>(pb + c0 + 16), b1 = *reinterpret_cast<const d2*>(pb + c0 + 18);
        c0v = *reinterpret_cast<const d2*>(pc + c0 + 16), c1v = *reinterpret_cast<const d2*>(pc + c0 + 18);
      }
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(x0[e], y0[e], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(x0[e], z0[e], acc1, 0, 0, 0);
      }
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(x1[e], y1[e], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(x1[e], z1[e], acc1, 0, 0, 0);
      }
    }
    // accumulator g of lane l: row (l >> 4) + 4 g, column l & 15
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int i = i0 + h + 4 * g;
      if (i < rows) {
        double* p = row(i) + j0 + m;
        p[0] -= acc0[g];
        p[16] -= acc1[g];
      }
    }
  }
}

#ifdef MGP_LARGE_VALU_UPDATE
// A/B copy of step 1 on the VALU (tools/mkvariant.sh valu mgp_large.hip -DMGP_LARGE_VALU_UPDATE=1):
// the same operands from the same place -- rows of L as 16-byte loads from the slab, nothing staged in LDS -- with a
// register tile of 8 rows x 4 panel columns per thread, the contraction in ascending column order.
template <typename T>
__device__ __forceinline__ void panel_update_valu(SlabRows<T> row, int j0, int rows, int tid, int NT) {
  using V = typename lds_vec<T>::type;
  constexpr int E = 16 / (int)sizeof(T), TM = 8, TN = 4;
  const int ntasks = (rows - j0 + TM - 1) / TM * (LNB / TN);
  for (int t = tid; t < ntasks; t += NT) {
    const int n0 = j0 + t % (LNB / TN) * TN, i0 = j0 + t / (LNB / TN) * TM;
    const T* pa[TM];
    const T* pb[TN];
#pragma unroll
    for (int i = 0; i < TM; ++i) pa[i] = row(min(i0 + i, rows - 1));
#pragma unroll
    for (int n = 0; n < TN; ++n) pb[n] = row(min(n0 + n, rows - 1));
    T acc[TM][TN] = {};
    for (int c = 0; c < j0; c += E) {
      V av[TM], bv[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i) av[i] = *reinterpret_cast<const V*>(pa[i] + c);
#pragma unroll
      for (int n = 0; n < TN; ++n) bv[n] = *reinterpret_cast<const V*>(pb[n] + c);
#pragma unroll
      for (int e = 0; e < E; ++e)
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int n = 0; n < TN; ++n) acc[i][n] += av[i][e] * bv[n][e];
    }
#pragma unroll
    for (int i = 0; i < TM; ++i)
      if (i0 + i < rows) {
        T* p = row(i0 + i) + n0;
#pragma unroll
        for (int n = 0; n < TN; ++n) p[n] -= acc[i][n];
      }
  }
}
#endif

// All NT threads of the workgroup call this on a filled slab (every write to it behind a barrier).  Lb: LNB * large_lp
// elements of LDS, 16-byte aligned.  Returns, to every thread, whether a non-positive / NaN pivot was met.  On return
// (behind a barrier) rows 0 .. k-1 hold L with the inverse pivots on the diagonal, row k holds z = L^-1 c and row
// k+1+r holds L^-1 y_r.
//
// Entries right of the diagonal inside a diagonal block (never initialised) are carried along by step 1 and by the
// register factorisation, and stay where they are: lane r's entry (r, c) with c > r only ever feeds entries (r, m)
// with m > c of the same lane, no broadcast reads them (the broadcast of column c takes lanes >= c), and step 3 reads
// row c of the block up to its diagonal.
template <typename T>
__device__ __forceinline__ bool factor_augmented_slab(SlabRows<T> row, int k, int rows, T* Lb, int tid, int NT) {
  using V = typename lds_vec<T>::type;
  constexpr int E = 16 / (int)sizeof(T);
  constexpr int LP = large_lp<T>();
  const int lane = tid & 63, r = lane & 31;
  bool bad = false;
  for (int j0 = 0; j0 < k; j0 += LNB) {
    const int nb = min(LNB, k - j0);
    if (j0 > 0) {
#ifdef MGP_LARGE_VALU_UPDATE
      panel_update_valu<T>(row, j0, rows, tid, NT);
#else
      panel_update(row, j0, rows, tid, NT);
#endif
      __syncthreads();
    }
    // step 2: row r of the diagonal block in lane r's registers; the block is padded to 32 x 32 with the identity
    // (a last panel of nb < 32 columns: the padding's pivots are 1 and it leaves the rest alone)
    {
      T D[LNB];
      T dinv = T(0);  // lane r: the inverse pivot of column r
      // (the lane index behind an empty asm, once per use: the 32 lane masks r == c are then made where they are
      // used instead of being hoisted out of the panel loop, kept in 64 scalar registers and spilled)
      int r1 = r, r2 = r, r3 = r;
      asm volatile("" : "+v"(r1));
      asm volatile("" : "+v"(r2));
      asm volatile("" : "+v"(r3));
      const T* src = row(min(j0 + r, rows - 1)) + j0;
#pragma unroll
      for (int c = 0; c < LNB; c += E) {
        const V v = *reinterpret_cast<const V*>(src + c);
#pragma unroll
        for (int e = 0; e < E; ++e) D[c + e] = (r < nb && c + e < nb) ? v[e] : (r1 == c + e ? T(1) : T(0));
      }
      __syncthreads();  // every wave holds the block: its rows (and the LDS copy of the last one) may now be overwritten
#pragma unroll
      for (int c = 0; c < LNB; ++c) {
        const T p = lane_value(D[c], c);
        bad = bad || !(p > T(0));
        const T iv = num<T>::rsqrt(p);
        const T v = D[c] * iv;  // lane r > c: L[r][c]
        D[c] = v;
        dinv = r2 == c ? iv : dinv;
        // (eight broadcasts at a time: left alone, the scheduler lines up the whole block's and spills scalars)
#pragma unroll
        for (int m = c + 1; m < LNB; ++m) {
          D[m] -= v * lane_value(v, m);
          if ((m & 7) == 7) __builtin_amdgcn_sched_barrier(0);
        }
      }
      if (tid < LNB) {  // the first wave's copy goes to the slab and, for step 3, to LDS
        T* dst = row(min(j0 + r, rows - 1)) + j0;
#pragma unroll
        for (int c = 0; c < LNB; c += E) {
          V v;
#pragma unroll
          for (int e = 0; e < E; ++e) v[e] = r3 == c + e ? dinv : D[c + e];  // (the diagonal keeps the inverse pivot)
          *reinterpret_cast<V*>(Lb + r * LP + c) = v;
          if (r < nb) *reinterpret_cast<V*>(dst + c) = v;
        }
      }
    }
    __syncthreads();
    // step 3: y = a L^-T for the 32 panel entries a of every row below the block, one row per thread; row c of the
    // block comes out of LDS as 16-byte broadcasts
    for (int i = j0 + nb + tid; i < rows; i += NT) {
      T* p = row(i) + j0;
      T y[LNB];
#pragma unroll
      for (int c = 0; c < LNB; c += E) {
        const V v = *reinterpret_cast<const V*>(p + c);
#pragma unroll
        for (int e = 0; e < E; ++e) y[c + e] = v[e];
      }
#pragma unroll
      for (int c = 0; c < LNB; ++c) {
        T v = y[c];
#pragma unroll
        for (int m0 = 0; m0 <= c; m0 += E) {
          const V l = *reinterpret_cast<const V*>(Lb + c * LP + m0);
#pragma unroll
          for (int e = 0; e < E; ++e) {
            if (m0 + e < c) v -= y[m0 + e] * l[e];
            if (m0 + e == c) v *= l[e];  // (the inverse pivot: the last entry the row contributes)
          }
        }
        y[c] = v;
        __builtin_amdgcn_sched_barrier(0);  // (one row of the block in flight, not all 32)
      }
#pragma unroll
      for (int c = 0; c < LNB; c += E) {
        V v;
#pragma unroll
        for (int e = 0; e < E; ++e) v[e] = y[c + e];
        *reinterpret_cast<V*>(p + c) = v;  // (columns past k of a last panel: inside the row, never read as data)
      }
    }
    __syncthreads();
  }
  return bad;
}

// Back-substitution L^T x = L^-1 y_r of all R responses at once behind a factorisation that left L^-1 y_r in rows
// k + 1 + r (factor_augmented_slab, factor_augmented_rows), on any row layout, in place, column by column from the
// last: x[j] = w[j] / L[j][j], then w[m] -= L[j][m] x[j] for every m < j -- row j of L, read contiguously by consecutive
// threads, one barrier per column.  inv_pivot(j) = 1 / L[j][j] (the slab keeps it on the diagonal, the LDS factor in a
// list of its own).  co: the (k, R) coefficients of this neighbourhood; NaN behind a bad pivot.  The first barrier
// stands between the caller's reads of the tail rows and their updates.
template <typename T, typename Rows, typename InvPivot>
__device__ __forceinline__ void back_substitute_columns(Rows row, int k, int R, InvPivot inv_pivot, bool bad, T* co, int tid, int NT) {
  for (int j = k - 1; j >= 0; --j) {
    __syncthreads();  // the outputs' reads / the updates of column j + 1 are done
    const T* Lj = row(j);
    const T ivj = inv_pivot(j);
    for (int r = tid; r < R; r += NT) co[j * (int64_t)R + r] = bad ? num<T>::nan() : row(k + 1 + r)[j] * ivj;
    for (int m = tid; m < j; m += NT) {
      const T l = Lj[m] * ivj;
      for (int r = 0; r < R; ++r) {
        T* w = row(k + 1 + r);
        w[m] -= l * w[j];
      }
    }
  }
}

}  // namespace mgp
