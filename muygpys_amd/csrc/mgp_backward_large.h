// The phases the two backward kernels on the slab factor share (mgp_backward_large.hip: the hyper-parameter partials;
// mgp_backward_large_full.hip: the whole vector-Jacobian product): the LDS carve, the assembly of a backward slab (out
// of the pieces of mgp_assemble.h, where the cotangent of a pair lives too), the back-substitution of its two tail
// rows, the per-feature length-scale sums of one feature chunk, and the launch rule.  Every sum here is per-thread partials in a fixed pair order -> wave_sum -> the waves'
// totals in wave order through LDS: no floating-point atomic.
#pragma once

#include "mgp_assemble.h"
#include "mgp_large_factor.h"

namespace mgp {

constexpr int kBwdGroup = 8;  // features summed per pass over the triangle
constexpr int kBwdMaxWaves = 8;

// the workgroup's total of v, to every thread, in a fixed order: lanes by the butterfly, waves in ascending order.
// red: kBwdMaxWaves elements of LDS.  Two barriers.
template <typename T>
__device__ __forceinline__ T block_sum_ordered(T v, T* red, int tid, int NT) {
  v = wave_sum(v);
  if ((tid & 63) == 0) red[tid >> 6] = v;
  __syncthreads();
  T s = red[0];
  for (int w = 1; w < (NT >> 6); ++w) s += red[w];
  __syncthreads();
  return s;
}

// dynamic LDS carve (every array 16-byte aligned; KA = k rounded up to a 16-byte piece):
// [Lb: LNB*LP T][idx: (k+2 & ~1) int64][X: (k+1)*XP T][il: dc T][av: KA T][wv: KA T][red: kBwdMaxWaves*kBwdGroup T]
template <typename T>
struct BackwardLargeLds {
  T* Lb;
  int64_t* idx;
  T *X, *il, *av, *wv, *red;
  int XP;
};

template <typename T>
__device__ __forceinline__ BackwardLargeLds<T> backward_large_carve(char* smem, int k, int dc) {
  constexpr int E = 16 / (int)sizeof(T);
  const int KA = (k + E - 1) / E * E;
  BackwardLargeLds<T> s;
  s.XP = tile_row_stride<T>(dc);
  s.Lb = reinterpret_cast<T*>(smem);
  s.idx = reinterpret_cast<int64_t*>(s.Lb + LNB * large_lp<T>());
  s.X = reinterpret_cast<T*>(s.idx + ((k + 2) & ~1));
  s.il = s.X + (k + 1) * s.XP;
  s.av = s.il + dc;
  s.wv = s.av + KA;
  s.red = s.wv + KA;
  return s;
}

template <typename T>
static size_t backward_large_lds_bytes(int k, int dc) {
  const int E = 16 / (int)sizeof(T);
  size_t n = (size_t)((k + 2) & ~1) * sizeof(int64_t);
  n += ((size_t)LNB * large_lp<T>() + (size_t)(k + 1) * (dc + E) + dc + 2 * (size_t)((k + E - 1) / E * E) +
        (size_t)kBwdMaxWaves * kBwdGroup) * sizeof(T);
  return (n + 15) & ~(size_t)15;
}

// the feature chunk and the LDS of a launch: dc as the forward (a multiple of 8, as wide as fits)
template <typename T>
static FeatureChunk backward_large_chunk(int k, int d) {
  return feature_chunk(d, [&](int dc) { return backward_large_lds_bytes<T>(k, dc); });
}

// ---- 1. the index list, squared distances (kept in Dst when keep_acc), covariances, nugget, the two tail rows: c, and
// ONE combined right-hand side yt = y (gyk given: the LOOCV form) or Y gm -- the pieces of mgp_assemble.h ----
template <typename T>
__device__ __forceinline__ void backward_large_assemble(const FusedArgs& a, const T* gmean, const T* gyk, bool keep_acc,
                                                        T post_scale, int64_t nb, int k, SlabRows<T> row, T* Dst,
                                                        const BackwardLargeLds<T>& s, int tid, int NT) {
  fill_index_list(s.idx, a, nb, k, tid, NT);
  __syncthreads();
  pair_distances<T>(a, k, s.idx, s.X, s.XP, s.il, tid, NT, [&](int p, int r, int c, T acc, int d0, bool last) {
    if (d0 > 0) acc += Dst[p];
    if (keep_acc) Dst[p] = acc;
    // the last chunk also writes the covariance into the system
    if (last) row(r)[c] = kernel_eval<T>(a.kernel_id, metric_arg<T>(acc, a.metric_id, post_scale));
  });
  fill_diagonal_and_rhs<T>(row, a, gmean, gyk, s.idx, nb, k, tid, NT);
  __syncthreads();
}

// ---- 3. back-substitution L^T [a w] = [z zy] of both tail rows, in LDS: column by column from the last, row j of L read
// contiguously with the inverse pivot on its diagonal; the chain of k dependent steps runs through LDS, and row j - 1
// of L is on its way from the slab while step j runs.  Leaves a = K^-1 c in av and w = K^-1 yt in wv ----
template <typename T>
__device__ __forceinline__ void backward_large_solve_tails(SlabRows<T> row, int k, T* av, T* wv, int tid, int NT) {
  constexpr int U = 2;  // entries of a tail row per thread: k <= 126 at 256 threads, k <= 1022 at 512
  for (int m = tid; m < k; m += NT) {
    av[m] = row(k)[m];
    wv[m] = row(k + 1)[m];
  }
  T ln[U], ivn, oa[U], ow[U];
  const T* Lj = row(k - 1);
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int m = tid + u * NT;
    ln[u] = m < k - 1 ? Lj[m] : T(0);
    oa[u] = ow[u] = T(0);
  }
  ivn = Lj[k - 1];
  __syncthreads();
  for (int j = k - 1; j >= 0; --j) {
    T l[U];
#pragma unroll
    for (int u = 0; u < U; ++u) l[u] = ln[u];
    const T iv = ivn;
    if (j > 0) {  // row j - 1 of L: nothing in it depends on this step
      const T* Ln = row(j - 1);
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int m = tid + u * NT;
        ln[u] = m < j - 1 ? Ln[m] : T(0);
      }
      ivn = Ln[j - 1];
    }
    const T xa = av[j] * iv, xw = wv[j] * iv;  // (entry j is final: steps > j are behind the barrier)
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int m = tid + u * NT;
      if (m < j) {
        av[m] -= l[u] * xa;
        wv[m] -= l[u] * xw;
      }
      if (m == j) oa[u] = xa, ow[u] = xw;  // its owner keeps the solution; written once nobody reads entry j
    }
    __syncthreads();
  }
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int m = tid + u * NT;
    if (m < k) av[m] = oa[u], wv[m] = ow[u];
  }
  __syncthreads();
}

// ---- 5. Anisotropy, one feature chunk whose rows are staged in X: grad_ls[c] = -2 / l_c^3 sum_pairs q_ij (x_ic - x_jc)^2
// with q_ij = qof(p, i, j) wherever the kernel keeps it, eight features per pass.  gls_row / ls: at the chunk's first
// feature ----
template <typename T, typename QOf>
__device__ __forceinline__ void pair_ls_chunk(QOf qof, const T* X, int XP, T* red, const T* ls, T* gls_row, int w, int wp,
                                              int npairs, int tid, int NT) {
  using V = typename lds_vec<T>::type;
  constexpr int E = 16 / (int)sizeof(T);
  for (int c0 = 0; c0 < wp; c0 += kBwdGroup) {
    V s[kBwdGroup / E];
#pragma unroll
    for (int u = 0; u < kBwdGroup / E; ++u) s[u] = V(0);
    for (int p = tid; p < npairs; p += NT) {
      int a_, c_;
      tri_decode(p, a_, c_);
      const T q = qof(p, a_, c_);
      const T* xa = X + a_ * XP + c0;
      const T* xc = X + c_ * XP + c0;
#pragma unroll
      for (int u = 0; u < kBwdGroup / E; ++u)
        if (c0 + u * E < wp) {  // uniform
          const V df = *reinterpret_cast<const V*>(xa + u * E) - *reinterpret_cast<const V*>(xc + u * E);
          s[u] += q * df * df;
        }
    }
#pragma unroll
    for (int u = 0; u < kBwdGroup / E; ++u)
#pragma unroll
      for (int e = 0; e < E; ++e) {
        const T v = wave_sum(s[u][e]);
        if ((tid & 63) == 0) red[(tid >> 6) * kBwdGroup + u * E + e] = v;
      }
    __syncthreads();
    if (tid < kBwdGroup && c0 + tid < w) {
      T t = red[tid];
      for (int wi = 1; wi < (NT >> 6); ++wi) t += red[wi * kBwdGroup + tid];
      const T ilc = T(1) / ls[c0 + tid];
      gls_row[c0 + tid] = T(-2) * ilc * ilc * ilc * t;
    }
    __syncthreads();
  }
}
// ... with q in the triangle Dst of a backward slab
template <typename T>
__device__ __forceinline__ void backward_large_ls_chunk(const T* Dst, const T* X, int XP, T* red, const T* ls, T* gls_row,
                                                        int w, int wp, int npairs, int tid, int NT) {
  pair_ls_chunk<T>([&](int p, int, int) { return Dst[p]; }, X, XP, red, ls, gls_row, w, wp, npairs, tid, NT);
}

}  // namespace mgp
