// Backward pass (vector-Jacobian product) of the fused local-GP path for the general-smoothness Matern (kernel_id
// MGP_KERNEL_MATERN_GEN, FusedArgs::smoothness): backward_kernel (mgp_backward.hip: the same system in LDS, the same
// factorisations, the same feature sweep, the same thread rule) with the kernel function and its derivatives taken
// from the in-kernel evaluators of mgp_wave_common.h, and one more output: grad_nu (b), the partial with respect to
// the smoothness.  What the reference gets from torch autograd over torch/muygps_layer.py:129-164 with _matern_gen_fn
// as the kernel function.
//
// What differs from backward_kernel, per neighbourhood:
//   - the squared distances stay in Q and the last feature chunk copies them into S, where gen_covariance_phase
//     (mgp_gen_launch.h) turns them into covariances in place
//   - the pair-cotangent phase is strip-mined like gen_covariance_phase -- the evaluators end their node loop on a wave
//     ballot, so every thread makes the same number of gen_deriv_strip calls; a strip = NT threads x 4 (fp32) / 2
//     (fp64) pairs, its map a function of k and NT alone; dead pairs are evaluated at x = 1 and never stored.  Per
//     live pair dk/dr and, NU, dk/dnu come from one call: q = gK dk_dacc goes into Q (mirrored, diagonal zeroed),
//     liso += gK kp x, lnu += gK dk/dnu.  A pair at zero distance gets 0 for both derivatives from the evaluators:
//     it contributes to no feature, length-scale or smoothness cotangent, also below nu = 1/2 where dk/dr diverges
//   - grad_ls, grad_noise and grad_nu of a neighbourhood are the same bits wherever it sits in a batch or a grid: the
//     isotropic sum and grad_nu are closed with block_sum_ordered, the per-feature sums with pair_ls_chunk
//     (mgp_backward_large.h: per-thread partials in a fixed pair order -> wave_sum -> the waves' totals in wave order),
//     no floating-point atomic in LDS.  The feature and response cotangents leave through global atomics as in
//     backward_kernel.
// LDS: backward_kernel's carve with the ordered sums' buffer in place of its two accumulators, behind it the node table
// of the forward and the derivative table (2 + 2 columns: 2 KiB in fp32, 8 KiB in fp64).
#include "mgp_args.h"
#include "mgp_assemble.h"
#include "mgp_backward_large.h"  // block_sum_ordered, pair_ls_chunk
#include "mgp_backward_lds.h"
#include "mgp_gen_launch.h"
#include "mgp_launch.h"

namespace mgp {

// dynamic LDS carve (every array up to colb 16-byte aligned; dc a multiple of 8):
// [idx (k+2 & ~1) i64][S (k+2)*SP][Q (k+1)*SP][X (k+1)*XP][il dc][colb 64][red kBwdMaxWaves*kBwdGroup][piv k][flag]
// [node table][derivative table]
template <typename T, bool NU>
__global__ __launch_bounds__(256) void backward_gen_kernel(BackwardArgs g, T* gnu, GenLaunch gl) {
  using V = typename lds_vec<T>::type;
  constexpr int E = 16 / (int)sizeof(T);
  constexpr int PC = gen_pairs_per_call<T>();
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const FusedArgs& a = g.f;
  const int k = a.k, d = a.d, R = a.R, dc = a.dc;
  const int rows = k + 2;
  const int SP = lds_row_stride<T>(k);
  const int XP = tile_row_stride<T>(dc);
  int64_t* idx = reinterpret_cast<int64_t*>(smem);
  T* S = reinterpret_cast<T*>(idx + ((k + 2) & ~1));
  T* Q = S + rows * SP;
  T* X = Q + (k + 1) * SP;
  T* il = X + (k + 1) * XP;
  T* colb = il + dc;  // 64-entry column broadcast buffer of the single-wave factorisation
  T* red = colb + 64;
  T* piv = red + kBwdMaxWaves * kBwdGroup;
  int* flag = reinterpret_cast<int*>(piv + k);
  const T* tab = reinterpret_cast<const T*>(smem + gl.tab);
  const T* dtab = reinterpret_cast<const T*>(smem + gl.dtab);

  const T* feat_q = static_cast<const T*>(a.feat_q);
  const T* feat_nn = static_cast<const T*>(a.feat_nn);
  const T* ls = static_cast<const T*>(a.length_scale);
  const T* gmean = static_cast<const T*>(g.grad_mean);
  const T* gvar = static_cast<const T*>(g.grad_var);
  const T* gyk = static_cast<const T*>(g.grad_yk);  // (LOOCV, R = 1: the right-hand side is y, w = gm u below)
  T* gq = static_cast<T*>(g.grad_feat_q);
  T* gnn = static_cast<T*>(g.grad_feat_nn);
  T* gtg = static_cast<T*>(g.grad_targets);
  T* gls = static_cast<T*>(g.grad_ls);
  T* gnz = static_cast<T*>(g.grad_noise);
  const int tid = threadIdx.x, NT = blockDim.x;
  const bool aniso = a.ls_count > 1;
  const bool l2 = a.metric_id == MGP_METRIC_L2;
  const int npairs = (k + 1) * k / 2;
  const bool vec_ok = d % E == 0 && dc % E == 0 && ((uintptr_t)feat_q | (uintptr_t)feat_nn) % 16 == 0;
  const bool sweep = gq || gnn || (gls && aniso);  // q of every pair is needed in Q

  const StridedRows<T> row{S, SP};
  const IsoScale<T> iso = iso_scale<T, true>(a);
  const T post_scale = iso.post_scale, inv_l = iso.inv_l;
  gen_build_node_table<T>(reinterpret_cast<T*>(smem + gl.tab), a.smoothness, gl, tid);
  gen_build_deriv_node_table<T>(reinterpret_cast<T*>(smem + gl.dtab), a.smoothness, gl, tid);

  for (int64_t nb = blockIdx.x; nb < a.b; nb += gridDim.x) {
    __syncthreads();  // previous neighbourhood fully consumed (first round: the tables are written)
    fill_index_list(idx, a, nb, k, tid, NT);
    __syncthreads();

    // ---- forward recomputation: acc (kept in Q, copied into S), covariances (S), combined right-hand side ----
    pair_distances<T>(a, k, idx, X, XP, il, tid, NT, [&](int, int r, int c, T acc, int d0, bool last) {
      T* dst = Q + r * SP + c;
      if (d0 > 0) acc += *dst;
      *dst = acc;
      if (last) S[r * SP + c] = acc;
    });
    // (each pair by the thread that wrote its distance: the strip map and pair_distances' both give pair p to p % NT)
    gen_covariance_phase<T>([&](int r, int c) { return S + r * SP + c; }, k, a.metric_id, post_scale, a.smoothness, gl, tab, tid, NT);
    fill_diagonal_and_rhs<T>(row, a, gmean, gyk, idx, nb, k, tid, NT);
    __syncthreads();
    const bool wave_path = NT == 64 && rows <= 64;  // uniform
    bool bad;
    if (wave_path) {
      bad = wave_factor_solve2<T>(S, SP, k, colb, tid);
    } else {
      bad = factor_augmented_lds<T>(S, SP, k, rows, piv, flag, tid, NT);
    }
    if (bad) {
      if (tid == 0 && a.info) atomicAdd(a.info, 1);
      continue;  // cotangents of a non-SPD neighbourhood are left untouched
    }
    T* av = S + k * SP;
    T* wv = S + (k + 1) * SP;
    if (!wave_path) {
      // ---- back-substitution L^T [a w] = [z zy], both vectors at once, column oriented ----
      for (int j = k - 1; j >= 0; --j) {
        if (tid < 2) S[(k + tid) * SP + j] *= piv[j];
        __syncthreads();
        const T aj = av[j], wj = wv[j];
        const T* Lj = S + j * SP;
        for (int m = tid; m < j; m += NT) {
          const T l = Lj[m];
          av[m] -= l * aj;
          wv[m] -= l * wj;
        }
        __syncthreads();
      }
    }
    const T gv = gvar ? gvar[nb] : T(0);
    // (LOOCV: wv holds u = K^-1 y; the mean's cotangent enters as the factor gm, y^T K^-1 y's as gyv)
    const T gyv = gyk ? gyk[nb] : T(0);
    const T gm1 = gyk ? (gmean ? gmean[nb] : T(0)) : T(1);

    // ---- cotangent of every pair's acc (overwrites Q), isotropic length-scale partial, smoothness partial ----
    if (sweep || gls || NU) {  // uniform
      T liso = T(0), lnu = T(0);
      for (int p0 = 0; p0 < npairs; p0 += NT * PC) {  // (uniform trip count)
        T v[PC], x[PC], dn[PC];
        int pa[PC], pc[PC];
        unsigned live = 0;
#pragma unroll
        for (int u = 0; u < PC; ++u) {
          const int p = p0 + u * NT + tid;
          v[u] = T(1);
          pa[u] = pc[u] = 0;
          if (p < npairs) {
            tri_decode(p, pa[u], pc[u]);
            v[u] = metric_arg<T>(Q[pa[u] * SP + pc[u]], a.metric_id, post_scale);
            live |= 1u << u;
          }
          x[u] = v[u];
          dn[u] = T(0);
        }
        gen_deriv_strip<T, NU>(v, dn, live, a.smoothness, gl, tab, dtab);
#pragma unroll
        for (int u = 0; u < PC; ++u) {
          if (!((live >> u) & 1u)) continue;
          const T gK = pair_cotangent<T>(av, wv, pa[u], pc[u], k, gv, gm1, gyv);
          const T kp = v[u];
          if (sweep) {  // uniform
            const T q = gK * dk_dacc<T>(x[u], kp, post_scale, l2);
            Q[pa[u] * SP + pc[u]] = q;  // symmetric, zero diagonal: the per-point sweep below runs a uniform loop
            Q[pc[u] * SP + pa[u]] = q;
          }
          liso += gK * kp * x[u];
          if constexpr (NU) lnu += gK * dn[u];
        }
      }
      for (int r = tid; r <= k; r += NT) Q[r * SP + r] = T(0);
      if (gls && !aniso) {
        const T total = block_sum_ordered<T>(liso, red, tid, NT);
        if (tid == 0) gls[nb] = -(l2 ? T(1) : T(2)) * inv_l * total;  // dx/dl = -x/l | -2x/l
      }
      if constexpr (NU) {
        const T total = block_sum_ordered<T>(lnu, red, tid, NT);
        if (tid == 0) gnu[nb] = total;
      }
    }
    if (gnz)
      for (int r = tid; r < k; r += NT) gnz[nb * k + r] = noise_cotangent<T>(av[r], wv[r], gv, gm1, gyv);
    if (gtg && (gmean || gyk))  // (LOOCV, R = 1: mean = a . y and y^T K^-1 y = y . u both read the responses)
      for (int t = tid; t < k * R; t += NT) {
        const int c = t / R, r = t - c * R;
        unsafeAtomicAdd(gtg + idx[c] * (int64_t)R + r,
                        (gmean ? gmean[nb * R + r] * av[c] : T(0)) + (gyk ? T(2) * gyv * wv[c] : T(0)));
      }

    // ---- per-point feature cotangents, per-feature length-scale partials ----
    if (!sweep) continue;
    for (int d0 = 0; d0 < d; d0 += dc) {
      const int w = min(dc, d - d0);
      const int wp = (w + E - 1) / E * E;
      __syncthreads();  // q is in Q; the previous chunk's rows are consumed
      gather_tile_lds<T>(X, XP, feat_q, feat_nn, idx, k, d, d0, w, wp, vec_ok, tid, NT);
      for (int c = tid; c < wp; c += NT) il[c] = c < w ? (aniso ? T(1) / ls[d0 + c] : T(1)) : T(0);
      __syncthreads();
      if (gq || gnn) {
        // one thread per (point, 16-byte piece of its row): q_ij is read once per four features
        const int pieces = wp / E;
        for (int t = tid; t < (k + 1) * pieces; t += NT) {
          const int i = t / pieces, c0 = (t - i * pieces) * E;
          const V xi = *reinterpret_cast<const V*>(X + i * XP + c0);
          const T* qi = Q + i * SP;
          V s = V(0);
#pragma unroll 2
          for (int j = 0; j <= k; ++j) s += qi[j] * (xi - *reinterpret_cast<const V*>(X + j * XP + c0));
          const V ilv = *reinterpret_cast<const V*>(il + c0);
          const V gx = T(2) * s * ilv * ilv;
          T* dst = i < k ? gnn : gq;
          if (dst == nullptr) continue;
#pragma unroll
          for (int e = 0; e < E; ++e)
            if (c0 + e < w) unsafeAtomicAdd(dst + idx[i] * (int64_t)d + d0 + c0 + e, gx[e]);
        }
      }
      // grad_ls[c] = -2 / l_c^3 sum_pairs q_ij (x_ic - x_jc)^2, every sum in a fixed order
      if (gls && aniso)
        pair_ls_chunk<T>([&](int, int r, int c) { return Q[r * SP + c]; }, X, XP, red, ls + d0,
                         gls + nb * (int64_t)a.ls_count + d0, w, wp, npairs, tid, NT);
    }
  }
}

// the LDS of a launch: the carve above and both node tables behind it
template <typename T>
static size_t backward_gen_carve_bytes(int k, int dc) {
  const int SP = lds_row_stride<T>(k);
  size_t n = (size_t)((k + 2) & ~1) * sizeof(int64_t);
  n += ((size_t)(k + 2) * SP + (size_t)(k + 1) * SP + (size_t)(k + 1) * (dc + 16 / sizeof(T)) + (size_t)dc + 64 +
        (size_t)kBwdMaxWaves * kBwdGroup + k) * sizeof(T) + 16;
  return (n + 15) & ~(size_t)15;
}
template <typename T>
static size_t backward_gen_lds_bytes(int k, int dc) {
  return backward_gen_carve_bytes<T>(k, dc) + gen_table_bytes(sizeof(T)) + gen_deriv_table_bytes(sizeof(T));
}

template <typename T>
int launch_backward_gen(const BackwardArgs& in, void* grad_nu, hipStream_t stream) {
  BackwardArgs g = in;
  if (g.f.k > max_nn_count_backward_gen(sizeof(T))) return MGP_EUNSUPPORTED;  // (k near INT_MAX must not reach the formula)
  const FeatureChunk fc = feature_chunk(g.f.d, [&](int dc) { return backward_gen_lds_bytes<T>(g.f.k, dc); });
  if (!fc.fits) return MGP_EUNSUPPORTED;
  g.f.dc = fc.dc;
  GenLaunch gl = gen_launch_constants(g.f.smoothness, sizeof(T) == 8);
  gl.tab = (int)backward_gen_carve_bytes<T>(g.f.k, fc.dc);
  gl.dtab = gl.tab + (int)gen_table_bytes(sizeof(T));
  const bool nu = grad_nu != nullptr;
  const int threads = g.f.k + 2 <= 64 ? 64 : (g.f.k + 2 <= 128 ? 128 : 256);
  const LaunchLabel label(g.f.b, g.f.k, g.f.d, g.f.R, "mgp::backward_gen_kernel<%s, %s> [threads=%d,dc=%d]",
                          sizeof(T) == 4 ? "float" : "double", nu ? "true" : "false", threads, fc.dc);
  if (nu)
    return launch_capacity(&backward_gen_kernel<T, true>, threads, fc.lds, g.f.b, Capacity{16}, stream, &label, g,
                           static_cast<T*>(grad_nu), gl).status;
  return launch_capacity(&backward_gen_kernel<T, false>, threads, fc.lds, g.f.b, Capacity{16}, stream, &label, g,
                         static_cast<T*>(nullptr), gl).status;
}

template int launch_backward_gen<float>(const BackwardArgs&, void*, hipStream_t);
template int launch_backward_gen<double>(const BackwardArgs&, void*, hipStream_t);

// the largest nn_count the entry serves: the narrowest feature chunk fits LDS next to both tables
int max_nn_count_backward_gen(int elem_size) {
  return largest_k([&](int k) {
    return (elem_size == 4 ? backward_gen_lds_bytes<float>(k, 8) : backward_gen_lds_bytes<double>(k, 8)) <= kCuLdsBytes;
  });
}

}  // namespace mgp
