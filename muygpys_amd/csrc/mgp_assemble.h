// The front end the LDS and slab workgroup kernels share, forward and backward (mgp_generic.hip, mgp_large.hip,
// mgp_backward.hip, mgp_backward_large.h): from the index list of a neighbourhood to its augmented system -- index list,
// feature chunks through LDS, squared distances of every pair, nugget, responses -- and the pieces the cotangent formulas
// of the backward kernels have in common; a model parameter that touches the assembly is written here once.  Where a
// value is stored is the caller's: rows come in through a row accessor (StridedRows, SlabRows), a pair's distance leaves
// through a callable.  Not included by the wave-sized kernels (fused_rhs*, fused_wide*, backward_wave, fast_mean,
// solve_wave: register-budgeted forms of their own) nor by any source the run-time compiler hashes (kSources, mgp_jit.hip).
#pragma once

#include "mgp_args.h"
#include "mgp_lds_factor.h"

namespace mgp {

// feature-tile row stride for a chunk of dc features (dc a multiple of 2E): 16-byte aligned rows, odd number of
// 16-byte slots
template <typename T>
__host__ __device__ inline int tile_row_stride(int dc) { return dc + 16 / (int)sizeof(T); }

// p -> (row, col) of the strict lower triangle of the (k+1)-point set (8 p + 1 is an exact float for every p here,
// p < 2^20; the two loops settle the last unit)
__device__ __forceinline__ void tri_decode(int p, int& row, int& col) {
  int a_ = (int)((1.0f + sqrtf(1.0f + 8.0f * (float)p)) * 0.5f);
  while (a_ * (a_ - 1) / 2 > p) --a_;
  while ((a_ + 1) * a_ / 2 <= p) ++a_;
  row = a_;
  col = p - a_ * (a_ - 1) / 2;
}

// Isotropy: post_scale multiplies a pair's summed squares (F2: 1 / l^2) or their root (l2: 1 / l) in front of the
// kernel function, inv_l = 1 / l is what d / dl of either needs; both 1 under Anisotropy (the scales are inside the
// sums).  The forward kernels divide once, 1 / (l l); the backward kernels square 1 / l -- the two differ in the last
// bit under F2, and each family keeps the bits it has always returned.
template <typename T>
struct IsoScale {
  T post_scale, inv_l;
};
// (`ls`: where the scale is read -- a.length_scale, or the row of a neighbourhood of an NS launch)
template <typename T, bool BACKWARD>
__device__ __forceinline__ IsoScale<T> iso_scale_at(const FusedArgs& a, const T* ls) {
  IsoScale<T> s{T(1), T(1)};
  if (a.ls_count > 1) return s;
  const T l = ls[0];
  const bool l2 = a.metric_id == MGP_METRIC_L2;
  if constexpr (BACKWARD) {
    s.inv_l = T(1) / l;
    s.post_scale = l2 ? s.inv_l : s.inv_l * s.inv_l;
  } else {  // (inv_l: not asked for)
    s.post_scale = l2 ? T(1) / l : T(1) / (l * l);
  }
  return s;
}
template <typename T, bool BACKWARD>
__device__ __forceinline__ IsoScale<T> iso_scale(const FusedArgs& a) {
  return iso_scale_at<T, BACKWARD>(a, static_cast<const T*>(a.length_scale));
}

// What a per-neighbourhood-scale (NS) instantiation of a workgroup kernel is handed next to FusedArgs: the (b, ls_count)
// length scales, row nb for the neighbourhood at position nb of the batch (NOT batch_idx[nb]).  FusedArgs::length_scale
// is not read by such an instantiation; every other instantiation receives no NsLaunch at all.
struct NsLaunch {
  const void* ls_batch;
};

// The scale(s) of neighbourhood nb of an NS launch: row nb of ls_batch, handed to iso_scale_at and pair_distances_at,
// which read it exactly as they read a launch-wide one (same loads, same divisions: a constant ls_batch gives the bits
// of the scalar launch).  *bad: whether some scale of the row is not finite and > 0 (NaN included) -- every thread walks
// the whole row (ls_count uniform loads, next to the (k+1) k / 2 pairs of the neighbourhood), so the answer is uniform
// across the workgroup without a barrier or LDS.
template <typename T>
__device__ __forceinline__ const T* ns_select_scales(const FusedArgs& a, const NsLaunch& n, int64_t nb, bool* bad) {
  const T* ls = static_cast<const T*>(n.ls_batch) + nb * a.ls_count;
  bool any = false;
  for (int c = 0; c < a.ls_count; ++c) {
    const T l = ls[c];
    any |= !(l > T(0) && l < num<T>::inf());
  }
  *bad = any;
  return ls;
}

// ... and what such a neighbourhood returns: NaN in every output it has and one count in info, like a non-positive pivot
template <typename T>
__device__ __forceinline__ void ns_refuse_neighbourhood(const FusedArgs& a, int64_t nb, int R, int tid, int NT) {
  T* mean = static_cast<T*>(a.mean);
  T* var = static_cast<T*>(a.var);
  T* yk = static_cast<T*>(a.ykinvy);
  for (int r = tid; r < R; r += NT) {
    if (mean) mean[nb * R + r] = num<T>::nan();
    if (yk) yk[nb * R + r] = num<T>::nan();
  }
  if (tid == 0) {
    if (var) var[nb] = num<T>::nan();
    if (a.info) atomicAdd(a.info, 1);
  }
}

// idx[0 .. k-1]: the neighbours' rows of feat_nn; idx[k]: the query's row of feat_q (batch_idx == NULL: row nb).
// Visible behind the caller's barrier.
__device__ __forceinline__ void fill_index_list(int64_t* idx, const FusedArgs& a, int64_t nb, int k, int tid, int NT) {
  for (int r = tid; r <= k; r += NT)
    idx[r] = r < k ? a.nn_idx[nb * k + r] : (a.batch_idx ? a.batch_idx[nb] : nb);
}
// ... of a launch without a query (the coefficient precompute, feat_q == feat_nn): the query slot is fed the first
// neighbour, whose row exists whatever b is; nothing of that slot is stored
__device__ __forceinline__ void fill_index_list_no_query(int64_t* idx, const FusedArgs& a, int64_t nb, int k, int tid, int NT) {
  for (int r = tid; r <= k; r += NT) idx[r] = a.nn_idx[nb * k + (r < k ? r : 0)];
}

// Squared (scaled, under Anisotropy) distances of the (k+1) k / 2 pairs of the (k+1)-point set, one chunk of a.dc
// features at a time: the chunk's rows are staged in X (row stride XP = tile_row_stride(dc)), the inverse length
// scales in il, and every pair's partial sum over the chunk's features is handed to
//   sink(p, row, col, acc, d0, last)     p: pair index; d0: the chunk's first feature; last: no chunk follows
// by the thread that owns the pair (p = tid, tid + NT, ...: the same thread in every chunk).  Summing over the chunks
// and turning the last sum into a covariance is the sink's: that is where the kernels differ.  Barriers: the caller's
// in front (idx written, X and il free), one behind every chunk.  `ls`: where the length scale(s) are read, as in
// iso_scale_at.
template <typename T, typename Sink>
__device__ __forceinline__ void pair_distances_at(const FusedArgs& a, const T* ls, int k, const int64_t* idx, T* X, int XP, T* il,
                                                  int tid, int NT, Sink sink) {
  using V = typename lds_vec<T>::type;
  constexpr int E = 16 / (int)sizeof(T);
  const int d = a.d, dc = a.dc;
  const T* feat_q = static_cast<const T*>(a.feat_q);
  const T* feat_nn = static_cast<const T*>(a.feat_nn);
  const bool aniso = a.ls_count > 1;
  const bool vec_ok = d % E == 0 && dc % E == 0 && ((uintptr_t)feat_q | (uintptr_t)feat_nn) % 16 == 0;
  const int npairs = (k + 1) * k / 2;
  for (int d0 = 0; d0 < d; d0 += dc) {
    const int w = min(dc, d - d0);
    const int wp = (w + E - 1) / E * E;  // zero-padded to whole 16-byte pieces
    // coalesced gather of the (k+1) x w feature tile: consecutive lanes walk a row
    gather_tile_lds<T>(X, XP, feat_q, feat_nn, idx, k, d, d0, w, wp, vec_ok, tid, NT);
    if (aniso)
      for (int c = tid; c < wp; c += NT) il[c] = c < w ? T(1) / ls[d0 + c] : T(0);
    __syncthreads();
    for (int p = tid; p < npairs; p += NT) {
      int a_, c_;
      tri_decode(p, a_, c_);
      const T* xa = X + a_ * XP;
      const T* xc = X + c_ * XP;
      T acc = T(0);
      if (aniso) {
#pragma unroll 2
        for (int j = 0; j < wp; j += E) {
          const V df = (*reinterpret_cast<const V*>(xa + j) - *reinterpret_cast<const V*>(xc + j)) *
                       *reinterpret_cast<const V*>(il + j);
          acc += vec_dot(df, df);
        }
      } else {
#pragma unroll 2
        for (int j = 0; j < wp; j += E) {
          const V df = *reinterpret_cast<const V*>(xa + j) - *reinterpret_cast<const V*>(xc + j);
          acc += vec_dot(df, df);
        }
      }
      sink(p, a_, c_, acc, d0, d0 + dc >= d);
    }
    __syncthreads();
  }
}
template <typename T, typename Sink>
__device__ __forceinline__ void pair_distances(const FusedArgs& a, int k, const int64_t* idx, T* X, int XP, T* il, int tid,
                                               int NT, Sink sink) {
  pair_distances_at<T>(a, static_cast<const T*>(a.length_scale), k, idx, X, XP, il, tid, NT, sink);
}

// the noise variance of neighbour r of neighbourhood nb: one scalar, a table by training row, or a (b, k) tensor
template <typename T>
__device__ __forceinline__ T nugget(const FusedArgs& a, const T* noise_dev, const int64_t* idx, int64_t nb, int k, int r) {
  if (a.noise_mode == MGP_NOISE_SCALAR) return (T)a.noise_scalar;
  if (a.noise_mode == MGP_NOISE_TABLE) return noise_dev[idx[r]];
  return noise_dev[nb * k + r];
}

// the diagonal of K + diag(eps): kernel(0) == 1 for every kernel on the path
template <typename T, typename Rows>
__device__ __forceinline__ void fill_diagonal(Rows row, const FusedArgs& a, const int64_t* idx, int64_t nb, int k, int tid, int NT) {
  const T* noise_dev = static_cast<const T*>(a.noise_dev);
  for (int r = tid; r < k; r += NT) row(r)[r] = T(1) + nugget<T>(a, noise_dev, idx, nb, k, r);
}

// the R responses of the k neighbours into the tail rows k + 1 .. k + R: out of the table by training row, or out of
// the gathered (b, k, R) tensor (targets_batch)
template <typename T, typename Rows>
__device__ __forceinline__ void fill_responses(Rows row, const FusedArgs& a, const int64_t* idx, int64_t nb, int k, int R, int tid, int NT) {
  const T* targets = static_cast<const T*>(a.targets);
  for (int t = tid; t < k * R; t += NT) {
    const int c = t / R, r = t - c * R;
    row(k + 1 + r)[c] = targets[(a.targets_batch ? nb * k + c : idx[c]) * (int64_t)R + r];
  }
}

// The backward kernels' form of the two: the diagonal, and in row k + 1 ONE combined right-hand side whatever R is --
// yt = y (gyk given: the LOOCV form, R = 1), Y gm (gmean given), or 0
template <typename T, typename Rows>
__device__ __forceinline__ void fill_diagonal_and_rhs(Rows row, const FusedArgs& a, const T* gmean, const T* gyk, const int64_t* idx,
                                                      int64_t nb, int k, int tid, int NT) {
  const T* targets = static_cast<const T*>(a.targets);
  const T* noise_dev = static_cast<const T*>(a.noise_dev);
  const int R = a.R;
  for (int r = tid; r < k; r += NT) {
    row(r)[r] = T(1) + nugget<T>(a, noise_dev, idx, nb, k, r);
    T yt = T(0);
    if (gyk)
      yt = targets[idx[r] * (int64_t)R];
    else if (gmean)
      for (int q = 0; q < R; ++q) yt += gmean[nb * R + q] * targets[idx[r] * (int64_t)R + q];
    row(k + 1)[r] = yt;
  }
}

// ---- cotangent pieces: a = K^-1 c in av, w = K^-1 yt in wv; gv, gm1, gyv the cotangents of the variance, of the mean
// (1 in the posterior form, where gm is inside yt) and of y^T K^-1 y ----

// d loss / d K_ac of the pair (a_, c_), a_ > c_, of the (k+1)-point set (point k is the query: d loss / d c)
template <typename T>
__device__ __forceinline__ T pair_cotangent(const T* av, const T* wv, int a_, int c_, int k, T gv, T gm1, T gyv) {
  const T ac = av[c_], wc = wv[c_];
  if (a_ < k) {
    const T aa = av[a_], wa = wv[a_];
    return T(2) * gv * aa * ac - gm1 * (aa * wc + ac * wa) - T(2) * gyv * wa * wc;
  }
  return gm1 * wc - T(2) * gv * ac;
}

// d kappa / d acc at the metric's argument x (kp = kappa'(x)): x = post_scale sqrt(acc) under l2 (a pair at zero distance
// contributes no distance gradient), post_scale acc under F2
template <typename T>
__device__ __forceinline__ T dk_dacc(T x, T kp, T post_scale, bool l2) {
  if (l2) return x > T(0) ? kp * post_scale * post_scale / (T(2) * x) : T(0);
  return kp * post_scale;
}

// d loss / d eps_r, the cotangent of a diagonal entry of K; without gm1 and gyv: the posterior form (gm1 = 1, no
// y^T K^-1 y), the same value without the multiplications by one and by zero
template <typename T>
__device__ __forceinline__ T noise_cotangent(T a, T w, T gv, T gm1, T gyv) {
  return gv * a * a - gm1 * a * w - gyv * w * w;
}
template <typename T>
__device__ __forceinline__ T noise_cotangent(T a, T w, T gv) {
  return gv * a * a - a * w;
}

}  // namespace mgp
