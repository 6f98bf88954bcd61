// The weak-lensing shear model (the reference's experimental ShearKernel / ShearKernel2in3out /
// ShearNoise33: gp/kernels/experimental/shear.py, _src/gp/kernels/shear/numpy.py, _src/gp/noise/numpy.py:30-53):
//   * shear_tensor_kernel: difference tensors (..., n, m, 2) -> the (..., I, n, O, m) block layouts
//   * solve_multi_kernel: the multi-output posterior of a materialised Kin (b, n, n) (mgp_solve_multi_*)
//   * shear_posterior_kernel: gather -> blocks -> nugget -> factor -> outputs in ONE launch
//     (mgp_shear_posterior_*), nothing of size (b, n, n) in HBM
//
// Each neighbour contributes `in` rows (kappa, gamma1, gamma2, or gamma1, gamma2), flattened
// component-major (row a * k + i), and the query contributes 3 rows of Kcross^T.  The system
//   rows 0 .. n-1 : K (n = in * k)      rows n .. n+2 : Kcross^T      row n+3 : the responses
// is held as a packed lower triangle in LDS (PackedRows, mgp_lds_factor.h): a padded square of
// 154 fp64 rows (k = 50) is ~190 KB and does not fit the 160 KiB of a CU, the triangle ~100 KB does.
// n elimination steps of factor_augmented_rows leave K_c^T K^-1 K_c, the 3 means and y^T K^-1 y as
// inner products of the trailing rows (emit_block_outputs): no back-substitution.
#include "mgp_args.h"
#include "mgp_assemble.h"
#include "mgp_launch.h"
#include "mgp_lds_factor.h"

namespace mgp {

// The 3 x 3 shear block at a difference (dx, dy), components (kappa, gamma1, gamma2).  All six
// functions share e = exp(-|d|^2 / (2 l)) / l^4; `ell` enters as the reference writes it, i.e. as a
// squared length.  Every entry is even in (dx, dy) and the block is symmetric.
template <typename T>
__device__ __forceinline__ void shear_block(T dx, T dy, T ell, T B[3][3]) {
  const T sx = dx * dx, sy = dy * dy, s = sx + sy, p = sx * sy, q = sx * sx + sy * sy, xy = dx * dy;
  const T il = T(1) / ell;
  const T e = num<T>::exp(-s * T(0.5) * il) * (il * il) * (il * il);
  const T l2 = ell * ell;
  B[0][0] = T(0.25) * (T(8) * l2 - T(8) * ell * s + T(2) * p + q) * e;  // kappa kappa
  B[0][1] = B[1][0] = T(0.25) * (T(6) * ell * (sy - sx) + (sx * sx - sy * sy)) * e;  // kappa gamma1
  B[0][2] = B[2][0] = T(0.5) * xy * (s - T(6) * ell) * e;  // kappa gamma2
  B[1][1] = T(0.25) * (T(4) * l2 - T(4) * ell * s - T(2) * p + q) * e;  // gamma1 gamma1
  B[1][2] = B[2][1] = T(0.5) * xy * (sx - sy) * e;  // gamma1 gamma2
  B[2][2] = (l2 - ell * s + p) * e;  // gamma2 gamma2
}

// out[g, a, i, c, j] = B(diffs[g, i, j])[3 - I + a][3 - O + c]: I = O = 3 the full 33 layout, I = O = 2
// the (gamma1, gamma2) sub-blocks, I = 2, O = 3 the gamma rows against all three query components.
// One thread per (g, i, j) writes that pair's whole block.
template <typename T, int I, int O>
__global__ void shear_tensor_kernel(const T* __restrict__ diffs, int64_t G, int n, int m, T ell, T* __restrict__ out) {
  const int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const int64_t nm = (int64_t)n * m;
  if (t >= G * nm) return;
  const int64_t g = t / nm;
  const int ij = (int)(t - g * nm), i = ij / m, j = ij - i * m;
  T B[3][3];
  shear_block<T>(diffs[2 * t], diffs[2 * t + 1], ell, B);
  T* o = out + g * (I * O) * nm;
#pragma unroll
  for (int a = 0; a < I; ++a)
#pragma unroll
    for (int c = 0; c < O; ++c) o[((int64_t)(a * n + i) * O + c) * m + j] = B[3 - I + a][3 - O + c];
}

// Row offsets of a packed system (k elimination columns, `rows` rows) into off[0 .. rows]; returns the
// element count.  Filled once per launch by one thread (off is tiny and the same for every neighbourhood).
template <typename T>
__host__ __device__ inline int packed_offsets(int k, int rows, int* off) {
  int s = 0;
  for (int i = 0; i < rows; ++i) {
    if (off) off[i] = s;
    s += packed_row_len<T>(i, k);
  }
  if (off) off[rows] = s;
  return s;
}

__host__ __device__ inline size_t align16(size_t n) { return (n + 15) & ~(size_t)15; }

// LDS carve: [S: packed (n + m + R) rows][piv: n T][off: rows + 1 int][flag]
template <typename T>
static size_t solve_multi_lds_bytes(int n, int m, int R) {
  const int rows = n + m + R;
  return align16((size_t)packed_offsets<T>(n, rows, nullptr) * sizeof(T)) + align16((size_t)n * sizeof(T)) +
         align16((size_t)(rows + 1) * sizeof(int)) + 16;
}

// LDS carve: [idx: (k+2 & ~1) int64][S: packed (n + 4) rows][pts: (k+1) x 2 T][piv: n T][off: rows + 1 int][flag]
template <typename T>
static size_t shear_lds_bytes(int k, int in) {
  const int n = in * k, rows = n + 4;
  return (size_t)((k + 2) & ~1) * sizeof(int64_t) + align16((size_t)packed_offsets<T>(n, rows, nullptr) * sizeof(T)) +
         align16((size_t)(k + 1) * 2 * sizeof(T)) + align16((size_t)n * sizeof(T)) +
         align16((size_t)(rows + 1) * sizeof(int)) + 16;
}

template <typename T>
__global__ void __launch_bounds__(256) solve_multi_kernel(SolveMultiArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int n = a.n, m = a.m, R = a.R, rows = n + m + R;
  const int tid = threadIdx.x, NT = blockDim.x;
  T* S = reinterpret_cast<T*>(smem);
  const int tot = packed_offsets<T>(n, rows, nullptr);
  T* piv = S + align16((size_t)tot * sizeof(T)) / sizeof(T);
  int* off = reinterpret_cast<int*>(piv + align16((size_t)n * sizeof(T)) / sizeof(T));
  int* flag = off + align16((size_t)(rows + 1) * sizeof(int)) / sizeof(int);
  if (tid == 0) packed_offsets<T>(n, rows, off);
  const PackedRows<T> row{S, off};
  const T* Kin = static_cast<const T*>(a.Kin);
  const T* Kc = static_cast<const T*>(a.Kcross);
  const T* Y = static_cast<const T*>(a.Y);

  for (int64_t nb = blockIdx.x; nb < a.b; nb += gridDim.x) {
    __syncthreads();  // the offsets are written / the previous neighbourhood is consumed
    const T* Kb = Kin + nb * (int64_t)n * n;
    for (int t = tid; t < n * n; t += NT) {
      const int i = t / n, j = t - i * n;
      if (j <= i) row(i)[j] = Kb[t];  // lower triangle, as LAPACK 'L' would read it
    }
    for (int t = tid; t < n * m; t += NT) {
      const int j = t / m, c = t - j * m;
      row(n + c)[j] = Kc[nb * (int64_t)n * m + t];
    }
    for (int t = tid; t < n * R; t += NT) {
      const int j = t / R, r = t - j * R;
      row(n + m + r)[j] = Y[nb * (int64_t)n * R + t];
    }
    __syncthreads();
    const bool bad = factor_augmented_rows<T>(row, n, rows, piv, flag, tid, NT);
    T* mean = static_cast<T*>(a.mean);
    T* kk = static_cast<T*>(a.kk);
    T* yk = static_cast<T*>(a.ykinvy);
    emit_block_outputs<T>(row, n, m, R, bad, kk ? kk + nb * m * m : nullptr, mean ? mean + nb * m * R : nullptr,
                          yk ? yk + nb * R : nullptr, tid, NT);
    if (bad && tid == 0 && a.info) atomicAdd(a.info, 1);
  }
}

// IN = 3: observes (kappa, gamma1, gamma2) (ShearKernel); IN = 2: observes (gamma1, gamma2) (ShearKernel2in3out).
// Observed component a is physical component P0 + a of the 3 x 3 block.
template <typename T, int IN>
__global__ void __launch_bounds__(256) shear_posterior_kernel(ShearArgs a) {
  constexpr int P0 = 3 - IN;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int k = a.k, n = IN * k, rows = n + 4;
  const int tid = threadIdx.x, NT = blockDim.x;
  int64_t* idx = reinterpret_cast<int64_t*>(smem);
  T* S = reinterpret_cast<T*>(idx + ((k + 2) & ~1));
  const int tot = packed_offsets<T>(n, rows, nullptr);
  T* pts = S + align16((size_t)tot * sizeof(T)) / sizeof(T);
  T* piv = pts + align16((size_t)(k + 1) * 2 * sizeof(T)) / sizeof(T);
  int* off = reinterpret_cast<int*>(piv + align16((size_t)n * sizeof(T)) / sizeof(T));
  int* flag = off + align16((size_t)(rows + 1) * sizeof(int)) / sizeof(int);
  if (tid == 0) packed_offsets<T>(n, rows, off);
  const PackedRows<T> row{S, off};

  const T* feat_q = static_cast<const T*>(a.feat_q);
  const T* feat_nn = static_cast<const T*>(a.feat_nn);
  const T* tg = static_cast<const T*>(a.targets);
  const T ell = (T)a.length_scale, eps = (T)a.noise;
  T B0[3][3];
  shear_block<T>(T(0), T(0), ell, B0);  // the 33 block at zero difference: diag(2, 1, 1) / l^2
  T nug[IN];
#pragma unroll
  for (int c = 0; c < IN; ++c) nug[c] = B0[P0 + c][P0 + c] + ((a.noise_mode == MGP_SHEAR_NOISE_33 && P0 + c == 0) ? T(2) * eps : eps);
  const int npairs = (k + 1) * k / 2;

  for (int64_t nb = blockIdx.x; nb < a.b; nb += gridDim.x) {
    __syncthreads();  // the offsets are written / the previous neighbourhood is consumed
    for (int r = tid; r <= k; r += NT) {
      const int64_t g = r < k ? a.nn_idx[nb * k + r] : (a.batch_idx ? a.batch_idx[nb] : nb);
      const T* src = (r < k ? feat_nn : feat_q) + 2 * g;
      idx[r] = g;
      pts[2 * r] = src[0];
      pts[2 * r + 1] = src[1];
    }
    __syncthreads();
    // strictly lower pairs (i, j), i > j, of the k + 1 points (point k = the query): one exp per pair
    for (int p = tid; p < npairs; p += NT) {
      int i, j;
      tri_decode(p, i, j);
      T B[3][3];
      shear_block<T>(pts[2 * i] - pts[2 * j], pts[2 * i + 1] - pts[2 * j + 1], ell, B);
      if (i < k) {
        // K[a k + i][c k + j] = B[a][c]; entries above the diagonal go to their mirror (B symmetric, even)
#pragma unroll
        for (int ra = 0; ra < IN; ++ra)
#pragma unroll
          for (int ca = 0; ca < IN; ++ca) {
            const int r1 = ra * k + i, c1 = ca * k + j;
            const T v = B[P0 + ra][P0 + ca];
            if (r1 >= c1) row(r1)[c1] = v;
            else row(c1)[r1] = v;
          }
      } else {
        // Kcross^T: row n + o (query component o), column c k + j
#pragma unroll
        for (int o = 0; o < 3; ++o)
#pragma unroll
          for (int ca = 0; ca < IN; ++ca) row(n + o)[ca * k + j] = B[P0 + ca][o];
      }
    }
    // the diagonal blocks (zero difference) with the nugget, and the responses
    for (int i = tid; i < k; i += NT) {
#pragma unroll
      for (int ra = 0; ra < IN; ++ra)
#pragma unroll
        for (int ca = 0; ca <= ra; ++ca) row(ra * k + i)[ca * k + i] = ra == ca ? nug[ra] : B0[P0 + ra][P0 + ca];
    }
    for (int t = tid; t < n; t += NT) {
      const int c = t / k, j = t - c * k;
      row(n + 3)[t] = a.targets_batch ? tg[(nb * IN + c) * (int64_t)k + j] : tg[idx[j] * a.targets_stride + c];
    }
    __syncthreads();
    const bool bad = factor_augmented_rows<T>(row, n, rows, piv, flag, tid, NT);
    T* mean = static_cast<T*>(a.mean);
    T* kk = static_cast<T*>(a.kk);
    T* yk = static_cast<T*>(a.ykinvy);
    emit_block_outputs<T>(row, n, 3, 1, bad, kk ? kk + nb * 9 : nullptr, mean ? mean + nb * 3 : nullptr,
                          yk ? yk + nb : nullptr, tid, NT);
    if (bad && tid == 0 && a.info) atomicAdd(a.info, 1);
  }
}

template <typename T>
int launch_shear_tensor(const T* diffs, int64_t G, int n, int m, int variant, double ell, T* out, hipStream_t stream) {
  const int64_t total = G * n * m;
  if (total == 0) return MGP_OK;
  const int NT = 256;
  const dim3 grid((unsigned)((total + NT - 1) / NT));
  if (variant == MGP_SHEAR_33)
    hipLaunchKernelGGL((shear_tensor_kernel<T, 3, 3>), grid, dim3(NT), 0, stream, diffs, G, n, m, (T)ell, out);
  else if (variant == MGP_SHEAR_KIN23)
    hipLaunchKernelGGL((shear_tensor_kernel<T, 2, 2>), grid, dim3(NT), 0, stream, diffs, G, n, m, (T)ell, out);
  else
    hipLaunchKernelGGL((shear_tensor_kernel<T, 2, 3>), grid, dim3(NT), 0, stream, diffs, G, n, m, (T)ell, out);
  MGP_HIP_CHECK_LAUNCH();
  return MGP_OK;
}

// (the persistent kernels: at most 16 workgroups per CU, as the workgroup kernels of mgp_generic.hip)
template <typename T>
int launch_solve_multi(const SolveMultiArgs& a, hipStream_t stream) {
  if ((int64_t)a.n + a.m + a.R > 4096) return MGP_EUNSUPPORTED;
  const size_t lds = solve_multi_lds_bytes<T>(a.n, a.m, a.R);
  if (lds > kCuLdsBytes) return MGP_EUNSUPPORTED;
  const LaunchLabel label(a.b, a.n, -1, a.R, "mgp::solve_multi_kernel<%s>", sizeof(T) == 4 ? "float" : "double");
  return launch_capacity(&solve_multi_kernel<T>, lds_factor_threads(a.n + a.m + a.R), lds, a.b, Capacity{16}, stream, &label, a).status;
}

template <typename T>
int launch_shear_posterior(const ShearArgs& a, hipStream_t stream) {
  // (sizing is O(rows) host work per call; a packed system of more than 4096 rows is tens of MB: refused outright)
  if ((int64_t)a.k * a.in_count > 4096) return MGP_EUNSUPPORTED;
  const size_t lds = shear_lds_bytes<T>(a.k, a.in_count);
  if (lds > kCuLdsBytes) return MGP_EUNSUPPORTED;
  const LaunchLabel label(a.b, a.k, -1, -1, "mgp::shear_posterior_kernel<%s,%d>", sizeof(T) == 4 ? "float" : "double", a.in_count);
  const auto kernel = a.in_count == 3 ? &shear_posterior_kernel<T, 3> : &shear_posterior_kernel<T, 2>;
  return launch_capacity(kernel, lds_factor_threads(a.in_count * a.k + 4), lds, a.b, Capacity{16}, stream, &label, a).status;
}

int shear_max_nn_count(int elem_size, int in_count) {
  return largest_k([&](int k) { return (elem_size == 4 ? shear_lds_bytes<float>(k, in_count) : shear_lds_bytes<double>(k, in_count)) <= kCuLdsBytes; });
}

template int launch_shear_tensor<float>(const float*, int64_t, int, int, int, double, float*, hipStream_t);
template int launch_shear_tensor<double>(const double*, int64_t, int, int, int, double, double*, hipStream_t);
template int launch_solve_multi<float>(const SolveMultiArgs&, hipStream_t);
template int launch_solve_multi<double>(const SolveMultiArgs&, hipStream_t);
template int launch_shear_posterior<float>(const ShearArgs&, hipStream_t);
template int launch_shear_posterior<double>(const ShearArgs&, hipStream_t);

}  // namespace mgp
