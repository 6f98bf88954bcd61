// Hyper-parameter backward for local systems beyond LDS (k + 2 <= kLargeMaxRows): the length-scale and noise partials
// of mgp_backward.hip -- same formulas, no feature or response cotangents -- on the slab and the blocked factor of
// mgp_large_factor.h.  One workgroup per neighbourhood on a persistent grid, one backward slab of a caller-provided
// workspace per workgroup; the only cross-workgroup atomic is the one on *info.
//
// Backward slab: [factor trapezoid of k + 2 rows: K + diag(eps), c, yt][strict lower triangle of the (k+1)-point set,
// row after row: acc of every pair, later its cotangent q], each region in whole 256-byte lines.  The query is the
// training row batch_idx[nb]: one table serves both sides, as in LOOCV.
//
// Per neighbourhood:
//   1. assemble as fused_large_kernel does (feature chunks of dc columns through LDS); the squared distances
//      accumulate in the triangle and stay there, the last chunk writes the covariances into the trapezoid.  Two tail
//      rows whatever R is: c, and ONE combined right-hand side yt = y (LOOCV form) or Y gm
//   2. factor_augmented_slab, unchanged
//   3. back-substitution L^T [a w] = [z zy] by the scheme of solve_large_kernel's coefficient output (column by column
//      from the last, row j of L read contiguously, the inverse pivot on its diagonal) with both tail rows in LDS: the
//      chain of k dependent steps runs through LDS, and row j - 1 of L is on its way from the slab while step j runs
//   4. cotangent of every pair (mgp_backward.hip), grad_noise, the isotropic length-scale sum
//   5. Anisotropy: the triangle now holds q = gK dkappa/dacc; per feature chunk the rows are staged in LDS again and
//      eight features at a time are summed over all pairs
// Every sum is per-thread partials in a fixed pair order -> wave_sum -> the waves' totals in wave order through LDS:
// no floating-point atomic, so what a neighbourhood returns depends on nothing but its own inputs (the block size is
// a function of k alone).
#include "mgp_large_factor.h"

namespace mgp {

constexpr int kBwdGroup = 8;  // features summed per pass over the triangle (Anisotropy)
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
__global__ void __launch_bounds__(512) hyper_backward_large_kernel(BackwardArgs g, T* workspace, int slab_elems, int factor_elems) {
  using V = typename lds_vec<T>::type;
  constexpr int E = 16 / (int)sizeof(T);
  constexpr int U = 2;  // entries of a tail row per thread: k <= 126 at 256 threads, k <= 1022 at 512
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const FusedArgs& a = g.f;
  const int k_ = a.k, d = a.d, R = a.R, dc = a.dc;
  const int XP = dc + E;
  const int KA = (k_ + E - 1) / E * E;
  T* Lb = reinterpret_cast<T*>(smem);
  int64_t* idx = reinterpret_cast<int64_t*>(Lb + LNB * large_lp<T>());
  T* X = reinterpret_cast<T*>(idx + ((k_ + 2) & ~1));
  T* il = X + (k_ + 1) * XP;
  T* av = il + dc;
  T* wv = av + KA;
  T* red = wv + KA;

  const T* feat = static_cast<const T*>(a.feat_nn);
  const T* targets = static_cast<const T*>(a.targets);
  const T* noise_dev = static_cast<const T*>(a.noise_dev);
  const T* ls = static_cast<const T*>(a.length_scale);
  const T* gmean = static_cast<const T*>(g.grad_mean);
  const T* gvar = static_cast<const T*>(g.grad_var);
  const T* gyk = static_cast<const T*>(g.grad_yk);
  T* gls = static_cast<T*>(g.grad_ls);
  T* gnz = static_cast<T*>(g.grad_noise);
  const int tid = threadIdx.x, NT = blockDim.x;
  const bool aniso = a.ls_count > 1;
  const bool l2 = a.metric_id == MGP_METRIC_L2;
  const bool vec_ok = d % E == 0 && dc % E == 0 && (uintptr_t)feat % 16 == 0;
  // the distances are read again by the next feature chunk and by the length-scale cotangents: a grad_noise-only call
  // whose features fit one chunk stores none
  const bool keep_acc = gls != nullptr || d > dc;

  T post_scale = T(1), inv_l = T(1);
  if (!aniso) {
    inv_l = T(1) / ls[0];
    post_scale = l2 ? inv_l : inv_l * inv_l;
  }

  for (int64_t nb = blockIdx.x; nb < a.b; nb += gridDim.x) {
    __syncthreads();  // previous neighbourhood fully consumed
    int k = k_;
    asm volatile("" : "+s"(k));
    const int rows = k + 2;
    const int npairs = (k + 1) * k / 2;
    T* slab = workspace + (int64_t)blockIdx.x * slab_elems;
    const SlabRows<T> row{slab, k};
    T* Dst = slab + factor_elems;
    for (int r = tid; r <= k; r += NT)
      idx[r] = r < k ? a.nn_idx[nb * k + r] : (a.batch_idx ? a.batch_idx[nb] : nb);
    __syncthreads();

    // ---- 1. squared distances (kept in Dst), covariances, nugget, the two tail rows ----
    for (int d0 = 0; d0 < d; d0 += dc) {
      const int w = min(dc, d - d0);
      const int wp = (w + E - 1) / E * E;  // zero-padded to whole 16-byte pieces
      gather_tile_lds<T>(X, XP, feat, feat, idx, k, d, d0, w, wp, vec_ok, tid, NT);
      if (aniso)
        for (int c = tid; c < wp; c += NT) il[c] = c < w ? T(1) / ls[d0 + c] : T(0);
      __syncthreads();
      for (int p = tid; p < npairs; p += NT) {
        int a_, c_;
        large_tri_decode(p, a_, c_);
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
        if (d0 > 0) acc += Dst[p];
        if (keep_acc) Dst[p] = acc;
        // the last chunk also writes the covariance into the system
        if (d0 + dc >= d) row(a_)[c_] = kernel_eval<T>(a.kernel_id, metric_arg<T>(acc, a.metric_id, post_scale));
      }
      __syncthreads();
    }
    for (int r = tid; r < k; r += NT) {
      T eps;
      if (a.noise_mode == MGP_NOISE_SCALAR) eps = (T)a.noise_scalar;
      else if (a.noise_mode == MGP_NOISE_TABLE) eps = noise_dev[idx[r]];
      else eps = noise_dev[nb * k + r];
      row(r)[r] = T(1) + eps;  // kernel(0) == 1 for every kernel on the path
      T yt = T(0);
      if (gyk)
        yt = targets[idx[r] * (int64_t)R];
      else if (gmean)
        for (int q = 0; q < R; ++q) yt += gmean[nb * R + q] * targets[idx[r] * (int64_t)R + q];
      row(k + 1)[r] = yt;
    }
    __syncthreads();

    // ---- 2. factorisation; rows k, k + 1 then hold z = L^-1 c and zy = L^-1 yt ----
    const bool bad = factor_augmented_slab<T>(row, k, rows, Lb, tid, NT);
    if (bad) {  // uniform
      if (tid == 0 && a.info) atomicAdd(a.info, 1);
      continue;  // the partials of a non-SPD neighbourhood are left untouched
    }

    // ---- 3. back-substitution of both tail rows, in LDS ----
    for (int m = tid; m < k; m += NT) {
      av[m] = row(k)[m];
      wv[m] = row(k + 1)[m];
    }
    {
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

    // ---- 4. cotangents: a = K^-1 c in av, w = K^-1 yt in wv ----
    const T gv = gvar ? gvar[nb] : T(0);
    const T gyv = gyk ? gyk[nb] : T(0);
    const T gm1 = gyk ? (gmean ? gmean[nb] : T(0)) : T(1);
    if (gls) {
      T liso = T(0);
      for (int p = tid; p < npairs; p += NT) {
        int a_, c_;
        large_tri_decode(p, a_, c_);
        const T ac = av[c_], wc = wv[c_];
        T gK;
        if (a_ < k) {
          const T aa = av[a_], wa = wv[a_];
          gK = T(2) * gv * aa * ac - gm1 * (aa * wc + ac * wa) - T(2) * gyv * wa * wc;
        } else {
          gK = gm1 * wc - T(2) * gv * ac;
        }
        const T x = metric_arg<T>(Dst[p], a.metric_id, post_scale);
        const T kp = kernel_deriv<T>(a.kernel_id, x);
        if (aniso) {
          T dk_dacc;
          if (l2) dk_dacc = x > T(0) ? kp * post_scale * post_scale / (T(2) * x) : T(0);
          else dk_dacc = kp * post_scale;
          Dst[p] = gK * dk_dacc;
        } else {
          liso += gK * kp * x;
        }
      }
      if (!aniso) {
        const T total = block_sum_ordered<T>(liso, red, tid, NT);
        if (tid == 0) gls[nb] = -(l2 ? T(1) : T(2)) * inv_l * total;  // dx/dl = -x/l | -2x/l
      }
    }
    if (gnz)
      for (int r = tid; r < k; r += NT) gnz[nb * k + r] = gv * av[r] * av[r] - gm1 * av[r] * wv[r] - gyv * wv[r] * wv[r];
    if (!(gls && aniso)) continue;  // uniform

    // ---- 5. Anisotropy: grad_ls[c] = -2 / l_c^3 sum_pairs q_ij (x_ic - x_jc)^2 ----
    for (int d0 = 0; d0 < d; d0 += dc) {
      const int w = min(dc, d - d0);
      const int wp = (w + E - 1) / E * E;
      __syncthreads();  // q is in the triangle; the previous chunk's rows are consumed
      gather_tile_lds<T>(X, XP, feat, feat, idx, k, d, d0, w, wp, vec_ok, tid, NT);
      __syncthreads();
      for (int c0 = 0; c0 < wp; c0 += kBwdGroup) {
        V s[kBwdGroup / E];
#pragma unroll
        for (int u = 0; u < kBwdGroup / E; ++u) s[u] = V(0);
        for (int p = tid; p < npairs; p += NT) {
          int a_, c_;
          large_tri_decode(p, a_, c_);
          const T q = Dst[p];
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
          const T ilc = T(1) / ls[d0 + c0 + tid];
          gls[nb * (int64_t)a.ls_count + d0 + c0 + tid] = T(-2) * ilc * ilc * ilc * t;
        }
        __syncthreads();
      }
    }
  }
}

template <typename T>
static size_t backward_large_lds_bytes(int k, int dc) {
  const int E = 16 / (int)sizeof(T);
  size_t n = (size_t)((k + 2) & ~1) * sizeof(int64_t);
  n += ((size_t)LNB * large_lp<T>() + (size_t)(k + 1) * (dc + E) + dc + 2 * (size_t)((k + E - 1) / E * E) +
        (size_t)kBwdMaxWaves * kBwdGroup) * sizeof(T);
  return (n + 15) & ~(size_t)15;
}

// the factor trapezoid with two tail rows, then the triangle of the (k+1)-point set: whole 256-byte lines each
int64_t backward_large_slab_bytes(int elem_size, int k) {
  const int64_t factor = large_slab_bytes(elem_size, k, 1);
  const int64_t tri = (int64_t)k * ((int64_t)k + 1) / 2;
  if (factor == INT64_MAX || tri > (INT64_MAX - factor - 255) / elem_size) return INT64_MAX;
  return factor + (tri * elem_size + 255) / 256 * 256;
}

int64_t backward_large_workspace_bytes(int elem_size, int k, int64_t b) {
  const int64_t slab = backward_large_slab_bytes(elem_size, k);
  int64_t n = b < 1 ? 1 : b;
  if (n > kCuCount * kMaxPerCu) n = kCuCount * kMaxPerCu;
  return n * slab > kMaxWorkspace ? kMaxWorkspace : n * slab;
}

template <typename T>
int launch_hyper_backward_large(const BackwardArgs& in, void* workspace, int64_t workspace_bytes, hipStream_t stream) {
  BackwardArgs g = in;
  const int64_t rows = (int64_t)g.f.k + 2;  // (64 bits: k near INT_MAX must not wrap past the limit)
  if (rows > kLargeMaxRows || g.f.kernel_id == MGP_KERNEL_MATERN_GEN) return MGP_EUNSUPPORTED;
  const int k = g.f.k;
  const int64_t slab = backward_large_slab_bytes(sizeof(T), k);
  int dc = g.f.d < 64 ? (g.f.d + 7) / 8 * 8 : 64;  // as the forward: a multiple of 8, as wide as fits
  while (dc > 8 && backward_large_lds_bytes<T>(k, dc) > kMaxLds) dc -= 8;
  const size_t lds = backward_large_lds_bytes<T>(k, dc);
  if (lds > kMaxLds) return MGP_EUNSUPPORTED;
  g.f.dc = dc;
  if (lds > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&hyper_backward_large_kernel<T>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return -(1000 + (int)e);
  }
  int64_t grid = workspace_bytes / slab;  // one workgroup per slab, at most one per CU, at most b
  if (grid > kCuCount * kMaxPerCu) grid = kCuCount * kMaxPerCu;
  if (grid > g.f.b) grid = g.f.b;
  hipLaunchKernelGGL(hyper_backward_large_kernel<T>, dim3((unsigned)grid), dim3(block_threads((int)rows)), lds, stream, g,
                     static_cast<T*>(workspace), (int)(slab / (int64_t)sizeof(T)),
                     (int)(large_slab_bytes(sizeof(T), k, 1) / (int64_t)sizeof(T)));
  MGP_HIP_CHECK_LAUNCH();
  note_launch("mgp::hyper_backward_large_kernel<%s>", sizeof(T) == 4 ? "float" : "double");
  return MGP_OK;
}

template int launch_hyper_backward_large<float>(const BackwardArgs&, void*, int64_t, hipStream_t);
template int launch_hyper_backward_large<double>(const BackwardArgs&, void*, int64_t, hipStream_t);

}  // namespace mgp
