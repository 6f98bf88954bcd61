// What the LDS workgroup backwards share (mgp_backward.hip: the closed-form kernels; mgp_backward_gen.hip: the
// general-smoothness Matern): the single-wave "factor, then solve for two right-hand sides".
#pragma once

#include "mgp_lds_factor.h"

namespace mgp {

// Single-wave form of "factor, then solve for two right-hand sides" (k + 2 <= 64 rows, 64 threads): the
// row-per-lane register elimination of mgp_fused_wave.hip (column broadcast through a 64-entry LDS
// buffer) on the system assembled in S, multipliers kept in S's lower triangle, then the
// back-substitution L^T [a w] = D^-1 L^-1 [c yt] with the finished component handed down by v_readlane.
// Leaves a = K^-1 c in row k and w = K^-1 yt in row k+1 of S, like the LDS path.  Returns "bad pivot".
template <typename T>
__device__ inline bool wave_factor_solve2(T* S, int SP, int k, T* colb, int lane) {
  constexpr int NP = 64;
  constexpr int E = 16 / (int)sizeof(T);
  using V = typename lds_vec<T>::type;
  const int rows = k + 2;
  V A[NP / E];
#pragma unroll
  for (int c4 = 0; c4 < NP / E; ++c4) A[c4] = V(0);
  if (lane < rows) {
    const T* src = S + lane * SP;
#pragma unroll
    for (int c4 = 0; c4 < NP / E; ++c4)
      if (c4 * E < k) A[c4] = *reinterpret_cast<const V*>(src + c4 * E);  // rows are 16-byte aligned, SP >= k + 1
  }
  bool bad = false;
#pragma unroll
  for (int j = 0; j < NP - 2; ++j) {
    if (j < k) {
      const T ajj = A[j / E][j % E];
      __syncthreads();
      colb[lane] = ajj;
      __syncthreads();
      const V cp = *reinterpret_cast<const V*>(colb + (j / E) * E);
      const T p = cp[j % E];
      bad = bad || !(p > T(0));
      const T t = lane > j && lane < rows ? ajj / p : T(0);
      if (lane > j && lane < rows) S[lane * SP + j] = t;  // multiplier l_ij (rows k, k+1: D^-1 L^-1 of the rhs)
      const V nt = V(-t);
      A[j / E] = cp * nt + A[j / E];
      constexpr int GC = sizeof(T) == 4 ? 8 : 4;
#pragma unroll
      for (int c0 = j / E + 1; c0 < NP / E; c0 += GC) {
        V cv[GC];
#pragma unroll
        for (int u = 0; u < GC; ++u)
          if (c0 + u < NP / E) cv[u] = *reinterpret_cast<const V*>(colb + (c0 + u) * E);
#pragma unroll
        for (int u = 0; u < GC; ++u)
          if (c0 + u < NP / E) A[c0 + u] = cv[u] * nt + A[c0 + u];
      }
    }
  }
  __syncthreads();
  // back-substitution, both vectors at once: lane j < k holds x_a(j), x_w(j)
  T xa = lane < k ? S[k * SP + lane] : T(0);
  T xw = lane < k ? S[(k + 1) * SP + lane] : T(0);
  for (int m = k - 1; m >= 1; --m) {
    const T am = __shfl(xa, m, 64), wm = __shfl(xw, m, 64);
    if (lane < m) {
      const T l = S[m * SP + lane];
      xa -= l * am;
      xw -= l * wm;
    }
  }
  __syncthreads();
  if (lane < k) {
    S[k * SP + lane] = xa;
    S[(k + 1) * SP + lane] = xw;
  }
  __syncthreads();
  return bad;
}

}  // namespace mgp
