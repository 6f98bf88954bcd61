// Fused fast posterior mean: prediction from precomputed coefficients.
//
// Reference workflow (src/MuyGPyS/examples/fast_posterior_mean.py:317-400,
// _src/gp/muygps/numpy.py:70-95, _src/gp/tensors/numpy.py:18-37,97-108): for every training
// point i the coefficients C_i = (K_i + eps)^-1 y_i of its self-including neighbourhood are
// computed once; a test point t then takes its closest training point c(t), that point's
// neighbourhood N = nn_fast[c(t)] and predicts
//
//      mean_t = sum_j kappa(dist(x_t, x_{N_j})) * C[c(t)][j]        (einsum 'ij,ijk->ik').
//
// The reference materialises crosswise differences (b,k,d), distances, Kcross (b,k) and the
// gathered coefficients; here one launch reads (k+1) feature rows + k*R coefficients per test
// point and writes R values: a pure gather kernel, HBM-bound by construction
// (algorithmic bytes per test point: (k+1) d s + k R s + 8 (k+2) + R s).
//
// One wave owns 64/NP test points at a time (NP = 32 or 64 slots >= k+1): rows are staged in
// LDS with the same row-walking 16-byte gather as the fused kernel, lane i then owns neighbour
// i: difference-form distance to the query row, kernel, product with its coefficient(s), and a
// cross-lane sum.
//
// Beyond 64 slots (any k, fast_mean_wide_kernel): one wave owns one test point and walks its neighbours in passes of
// 64 through the same tile; the covariances of all k neighbours wait in LDS and one cross-lane sum per response closes
// the point.  The wave-per-point form is the one kept for every k > 63: a workgroup-per-point form for the widest
// lists was not built -- the kernel moves (k+1) d s bytes per point whatever the form, and the persistent grid already
// holds sixteen independent waves per CU.
//
// The general-smoothness Matern (mgp_fast_posterior_mean_gen_*): kernels of their own behind the closed-form ones
// (fast_mean_gen_kernel, fast_mean_wide_gen_kernel), the same launches with the node table of the launch's smoothness
// in LDS behind everything else and the in-kernel evaluators in place of kernel_eval.
#include "mgp_args.h"
#include "mgp_gen_group.h"
#include "mgp_gen_launch.h"
#include "mgp_launch.h"

namespace mgp {

template <typename T> struct fv16;
template <> struct fv16<float> { typedef float type __attribute__((ext_vector_type(4))); static constexpr int N = 4; };
template <> struct fv16<double> { typedef double type __attribute__((ext_vector_type(2))); static constexpr int N = 2; };

struct FastArgs {
  const void* feat_q;
  const void* feat_nn;
  const int64_t* batch_idx;   // (b) rows of feat_q, NULL = identity
  const int64_t* nn_idx;      // (b, k) rows of feat_nn
  const void* coeffs;         // (n_train, k, R)
  const int64_t* coeff_row;   // (b) row of coeffs per test point (the closest training point)
  const void* length_scale;
  void* mean;                 // (b, R)
  int64_t b;
  int d, k, R, kernel_id, metric_id, ls_count;
  int dst, xs, vec_ok;
};

template <typename T, int NP>
__global__ __launch_bounds__(64) void fast_mean_kernel(FastArgs a) {
  constexpr int NH = 64 / NP;
  constexpr int E = fv16<T>::N;
  constexpr int CH = 2 * E;
  using V = typename fv16<T>::type;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int k = a.k, d = a.d, R = a.R, xs = a.xs, dst = a.dst;
  T* tile = reinterpret_cast<T*>(smem);                       // NH*NP rows x xs
  T* ilbuf = tile + NH * NP * xs;                             // dst
  int64_t* idxbuf = reinterpret_cast<int64_t*>(ilbuf + dst + (dst & 1));  // 64

  const T* feat_q = static_cast<const T*>(a.feat_q);
  const T* feat_nn = static_cast<const T*>(a.feat_nn);
  const T* coeffs = static_cast<const T*>(a.coeffs);
  const T* ls = static_cast<const T*>(a.length_scale);
  T* mean = static_cast<T*>(a.mean);
  const bool aniso = a.ls_count > 1;
  T post_scale = T(1);
  if (!aniso) {
    const T l = ls[0];
    post_scale = a.metric_id == MGP_METRIC_L2 ? T(1) / l : T(1) / (l * l);
  }

  const int lane = threadIdx.x;
  const int h = NH == 1 ? 0 : lane / NP;
  const int i = lane & (NP - 1);
  T* Xh = tile + h * NP * xs;
  int64_t* idxh = idxbuf + h * NP;
  const int64_t ntasks = (a.b + NH - 1) / NH;

  for (int64_t task = blockIdx.x; task < ntasks; task += gridDim.x) {
    const int64_t nb_raw = task * NH + h;
    const bool live = nb_raw < a.b;
    const int64_t nb = live ? nb_raw : a.b - 1;
    int64_t myidx = 0;
    if (i < k) myidx = a.nn_idx[nb * k + i];
    else if (i == k) myidx = a.batch_idx ? a.batch_idx[nb] : nb;
    const int64_t crow = a.coeff_row[nb];
    __syncthreads();
    idxh[i] = myidx * (int64_t)d;
    T acc = T(0);
    for (int d0 = 0; d0 < d; d0 += dst) {
      const int w = min(dst, d - d0);
      const int wp = (w + CH - 1) / CH * CH;
      __syncthreads();
      if (a.vec_ok) {
        const int c16 = w / E, c16p = wp / E;
        const int rpr = NP / c16p;
        const int sub = (int)(((unsigned)i * ((1u << 16) / (unsigned)c16p + 1u)) >> 16);
        const int c = i - sub * c16p;
        const bool lane_on = sub < rpr;
        constexpr int U = 6;
        for (int r0 = 0; r0 <= k; r0 += U * rpr) {
          V v[U];
#pragma unroll
          for (int u = 0; u < U; ++u) {
            const int row = r0 + u * rpr + sub;
            v[u] = V(0);
            if (lane_on && row <= k && c < c16)
              v[u] = *reinterpret_cast<const V*>((row < k ? feat_nn : feat_q) + idxh[row] + d0 + c * E);
          }
#pragma unroll
          for (int u = 0; u < U; ++u) {
            const int row = r0 + u * rpr + sub;
            if (lane_on && row <= k) *reinterpret_cast<V*>(Xh + row * xs + c * E) = v[u];
          }
        }
      } else {
        const unsigned magic = (1u << 20) / (unsigned)wp + 1u;
        for (int t = i; t < (k + 1) * wp; t += NP) {
          const int row = (int)(((unsigned)t * magic) >> 20);
          const int c = t - row * wp;
          Xh[row * xs + c] = c < w ? ((row < k ? feat_nn : feat_q) + idxh[row] + d0)[c] : T(0);
        }
      }
      if (aniso)
        for (int c = lane; c < wp; c += 64) ilbuf[c] = c < w ? T(1) / ls[d0 + c] : T(0);
      __syncthreads();
      if (i < k) {
        const T* xo = Xh + i * xs;
        const T* xq = Xh + k * xs;
        for (int c0 = 0; c0 < wp; c0 += E) {
          V df = *reinterpret_cast<const V*>(xq + c0) - *reinterpret_cast<const V*>(xo + c0);
          if (aniso) df = df * *reinterpret_cast<const V*>(ilbuf + c0);
#pragma unroll
          for (int e = 0; e < E; ++e) acc += df[e] * df[e];
        }
      }
    }
    T kv = T(0);
    if (i < k) kv = kernel_eval<T>(a.kernel_id, metric_arg<T>(acc, a.metric_id, post_scale));
    for (int r = 0; r < R; ++r) {
      T part = i < k ? kv * coeffs[(crow * k + i) * (int64_t)R + r] : T(0);
#pragma unroll
      for (int off = NP / 2; off > 0; off >>= 1) part += __shfl_xor(part, off, 64);
      if (live && i == 0) mean[nb * R + r] = part;
    }
  }
}

template <typename T, int NP>
static int launch_fast_np(FastArgs a, hipStream_t stream) {
  constexpr int NH = 64 / NP;
  constexpr int E = fv16<T>::N;
  constexpr int CH = 2 * E;
  const int dpad = (a.d + CH - 1) / CH * CH;
  a.dst = dpad < 64 ? dpad : 64;
  a.xs = a.dst + E;
  const uintptr_t align = (uintptr_t)a.feat_q | (uintptr_t)a.feat_nn;
  a.vec_ok = (a.d % E == 0) && (align % 16 == 0);
  size_t lds = ((size_t)NH * NP * a.xs + a.dst + (a.dst & 1)) * sizeof(T) + 64 * sizeof(int64_t);
  lds = (lds + 15) & ~(size_t)15;
  const int64_t ntasks = (a.b + NH - 1) / NH;
  int64_t grid = kAssumedCus * 16;  // memory-bound: grid-stride over plenty of resident waves
  if (grid > ntasks) grid = ntasks;
  hipLaunchKernelGGL((fast_mean_kernel<T, NP>), dim3((unsigned)grid), dim3(64), lds, stream, a);
  MGP_HIP_CHECK_LAUNCH();
  return MGP_OK;
}

// k + 1 > 64: one test point per wave, the neighbours in passes of 64 (lane i owns neighbours i, i + 64, ...).  Per
// feature chunk the query row is staged once (tile row 64) and every pass gathers its 64 neighbour rows into rows
// 0 .. 63 with the row-walking gather above; a neighbour's partial squared distance waits in kv[] between chunks (its
// own lane writes and reads it), the last chunk leaves the covariance there.  Then, per response, every lane sums its
// products over the passes and ONE cross-lane reduction closes the sum.
// The gather of a pass is fast_mean_kernel's, written out a second time with the pass's row count and source in place
// of (k + 1 rows, the query among them): sharing it as a device function would put the 32- and 64-slot instantiations
// through a new inlining decision, and their code is to stay what it was (same bits, same rate); a change to the
// gather's layout has to be made in both places.
// dynamic LDS carve: [idx: 64 int64][tile: 65 * xs T][il: dst T][kv: 64 ceil(k / 64) T]
template <typename T>
__global__ __launch_bounds__(64) void fast_mean_wide_kernel(FastArgs a) {
  constexpr int E = fv16<T>::N;
  constexpr int CH = 2 * E;
  using V = typename fv16<T>::type;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int k = a.k, d = a.d, R = a.R, xs = a.xs, dst = a.dst;
  const int npass = (k + 63) / 64;
  int64_t* idxbuf = reinterpret_cast<int64_t*>(smem);
  T* tile = reinterpret_cast<T*>(idxbuf + 64);
  T* xq = tile + 64 * xs;
  T* ilbuf = tile + 65 * xs;
  T* kv = ilbuf + dst;

  const T* feat_q = static_cast<const T*>(a.feat_q);
  const T* feat_nn = static_cast<const T*>(a.feat_nn);
  const T* coeffs = static_cast<const T*>(a.coeffs);
  const T* ls = static_cast<const T*>(a.length_scale);
  T* mean = static_cast<T*>(a.mean);
  const bool aniso = a.ls_count > 1;
  T post_scale = T(1);
  if (!aniso) {
    const T l = ls[0];
    post_scale = a.metric_id == MGP_METRIC_L2 ? T(1) / l : T(1) / (l * l);
  }
  const int lane = threadIdx.x;

  for (int64_t nb = blockIdx.x; nb < a.b; nb += gridDim.x) {
    const int64_t* nrow = a.nn_idx + nb * k;
    const T* qrow = feat_q + (a.batch_idx ? a.batch_idx[nb] : nb) * (int64_t)d;
    const int64_t crow = a.coeff_row[nb];
    for (int d0 = 0; d0 < d; d0 += dst) {
      const int w = min(dst, d - d0);
      const int wp = (w + CH - 1) / CH * CH;
      const bool last = d0 + dst >= d;
      __syncthreads();  // the tile's and kv's readers of the chunk / the test point before are done
      if (a.vec_ok) {
        if (lane < wp / E) *reinterpret_cast<V*>(xq + lane * E) = lane < w / E ? *reinterpret_cast<const V*>(qrow + d0 + lane * E) : V(0);
      } else {
        for (int c = lane; c < wp; c += 64) xq[c] = c < w ? qrow[d0 + c] : T(0);
      }
      if (aniso)
        for (int c = lane; c < wp; c += 64) ilbuf[c] = c < w ? T(1) / ls[d0 + c] : T(0);
      for (int p = 0; p < npass; ++p) {
        const int i = p * 64 + lane;
        const int nrows = min(64, k - p * 64);
        if (p > 0) __syncthreads();  // the pass before has read its rows
        idxbuf[lane] = i < k ? nrow[i] * (int64_t)d : 0;
        __syncthreads();
        if (a.vec_ok) {
          const int c16 = w / E, c16p = wp / E;
          const int rpr = 64 / c16p;
          const int sub = (int)(((unsigned)lane * ((1u << 16) / (unsigned)c16p + 1u)) >> 16);
          const int c = lane - sub * c16p;
          const bool lane_on = sub < rpr;
          constexpr int U = 6;
          for (int r0 = 0; r0 < nrows; r0 += U * rpr) {
            V v[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
              const int row = r0 + u * rpr + sub;
              v[u] = V(0);
              if (lane_on && row < nrows && c < c16) v[u] = *reinterpret_cast<const V*>(feat_nn + idxbuf[row] + d0 + c * E);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
              const int row = r0 + u * rpr + sub;
              if (lane_on && row < nrows) *reinterpret_cast<V*>(tile + row * xs + c * E) = v[u];
            }
          }
        } else {
          const unsigned magic = (1u << 20) / (unsigned)wp + 1u;
          for (int t = lane; t < nrows * wp; t += 64) {
            const int row = (int)(((unsigned)t * magic) >> 20);
            const int c = t - row * wp;
            tile[row * xs + c] = c < w ? (feat_nn + idxbuf[row] + d0)[c] : T(0);
          }
        }
        __syncthreads();
        if (i < k) {
          const T* xo = tile + lane * xs;
          T acc = d0 > 0 ? kv[i] : T(0);
          for (int c0 = 0; c0 < wp; c0 += E) {
            V df = *reinterpret_cast<const V*>(xq + c0) - *reinterpret_cast<const V*>(xo + c0);
            if (aniso) df = df * *reinterpret_cast<const V*>(ilbuf + c0);
#pragma unroll
            for (int e = 0; e < E; ++e) acc += df[e] * df[e];
          }
          kv[i] = last ? kernel_eval<T>(a.kernel_id, metric_arg<T>(acc, a.metric_id, post_scale)) : acc;
        }
      }
    }
    __syncthreads();
    const T* co = coeffs + crow * (int64_t)k * R;
    for (int r = 0; r < R; ++r) {
      T part = T(0);
      for (int i = lane; i < k; i += 64) part += kv[i] * co[i * (int64_t)R + r];
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) part += __shfl_xor(part, off, 64);
      if (lane == 0) mean[nb * R + r] = part;
    }
  }
}

template <typename T>
static int launch_fast_wide(FastArgs a, hipStream_t stream) {
  constexpr int E = fv16<T>::N;
  constexpr int CH = 2 * E;
  const int dpad = (a.d + CH - 1) / CH * CH;
  a.dst = dpad < 64 ? dpad : 64;
  a.xs = a.dst + E;
  const uintptr_t align = (uintptr_t)a.feat_q | (uintptr_t)a.feat_nn;
  a.vec_ok = (a.d % E == 0) && (align % 16 == 0);
  // at most 64 (8) + 65 * 66 + 64 + 1024 fp64 elements = 44 KiB (k <= 1023, the chunk of 64 features); d = 8, k = 100
  // in fp32: 4.4 KiB, as many waves per CU as the grid below asks for
  size_t lds = 64 * sizeof(int64_t) + ((size_t)65 * a.xs + a.dst + (size_t)(a.k + 63) / 64 * 64) * sizeof(T);
  lds = (lds + 15) & ~(size_t)15;
  int64_t grid = kAssumedCus * 16;  // memory-bound: grid-stride over plenty of resident waves
  if (grid > a.b) grid = a.b;
  hipLaunchKernelGGL((fast_mean_wide_kernel<T>), dim3((unsigned)grid), dim3(64), lds, stream, a);
  MGP_HIP_CHECK_LAUNCH();
  return MGP_OK;
}

// ---- the general-smoothness Matern ------------------------------------------------------------------------------------
// fast_mean_kernel with the covariance from the node table (byte g.tab of dynamic LDS, built once per workgroup before
// the task loop; nu and the launch constants: arguments of their own, FastArgs stays what the closed-form kernels take).
// The gather is written out a third time, under the policy stated above fast_mean_wide_kernel.  The evaluator ends its
// node loop on a wave ballot: every lane calls it, lanes without a neighbour (i >= k) with a cleared `live`.  With two
// test points in a wave (NP = 32) each half-wave sums to its own node count (mgp_gen_group.h): a point's bits do not
// depend on its partner.
template <typename T, int NP>
__global__ __launch_bounds__(64) void fast_mean_gen_kernel(FastArgs a, GenLaunch g, double nu) {
  constexpr int NH = 64 / NP;
  constexpr int E = fv16<T>::N;
  constexpr int CH = 2 * E;
  using V = typename fv16<T>::type;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int k = a.k, d = a.d, R = a.R, xs = a.xs, dst = a.dst;
  T* tile = reinterpret_cast<T*>(smem);                       // NH*NP rows x xs
  T* ilbuf = tile + NH * NP * xs;                             // dst
  int64_t* idxbuf = reinterpret_cast<int64_t*>(ilbuf + dst + (dst & 1));  // 64
  const T* gtab = reinterpret_cast<const T*>(smem + g.tab);

  const T* feat_q = static_cast<const T*>(a.feat_q);
  const T* feat_nn = static_cast<const T*>(a.feat_nn);
  const T* coeffs = static_cast<const T*>(a.coeffs);
  const T* ls = static_cast<const T*>(a.length_scale);
  T* mean = static_cast<T*>(a.mean);
  const bool aniso = a.ls_count > 1;
  T post_scale = T(1);
  if (!aniso) {
    const T l = ls[0];
    post_scale = a.metric_id == MGP_METRIC_L2 ? T(1) / l : T(1) / (l * l);
  }

  const int lane = threadIdx.x;
  const int h = NH == 1 ? 0 : lane / NP;
  const int i = lane & (NP - 1);
  T* Xh = tile + h * NP * xs;
  int64_t* idxh = idxbuf + h * NP;
  const int64_t ntasks = (a.b + NH - 1) / NH;
  gen_build_node_table<T>(reinterpret_cast<T*>(smem + g.tab), nu, g, lane);  // (visible behind the task loop's barriers)

  for (int64_t task = blockIdx.x; task < ntasks; task += gridDim.x) {
    const int64_t nb_raw = task * NH + h;
    const bool live = nb_raw < a.b;
    const int64_t nb = live ? nb_raw : a.b - 1;
    int64_t myidx = 0;
    if (i < k) myidx = a.nn_idx[nb * k + i];
    else if (i == k) myidx = a.batch_idx ? a.batch_idx[nb] : nb;
    const int64_t crow = a.coeff_row[nb];
    __syncthreads();
    idxh[i] = myidx * (int64_t)d;
    T acc = T(0);
    for (int d0 = 0; d0 < d; d0 += dst) {
      const int w = min(dst, d - d0);
      const int wp = (w + CH - 1) / CH * CH;
      __syncthreads();
      if (a.vec_ok) {
        const int c16 = w / E, c16p = wp / E;
        const int rpr = NP / c16p;
        const int sub = (int)(((unsigned)i * ((1u << 16) / (unsigned)c16p + 1u)) >> 16);
        const int c = i - sub * c16p;
        const bool lane_on = sub < rpr;
        constexpr int U = 6;
        for (int r0 = 0; r0 <= k; r0 += U * rpr) {
          V v[U];
#pragma unroll
          for (int u = 0; u < U; ++u) {
            const int row = r0 + u * rpr + sub;
            v[u] = V(0);
            if (lane_on && row <= k && c < c16)
              v[u] = *reinterpret_cast<const V*>((row < k ? feat_nn : feat_q) + idxh[row] + d0 + c * E);
          }
#pragma unroll
          for (int u = 0; u < U; ++u) {
            const int row = r0 + u * rpr + sub;
            if (lane_on && row <= k) *reinterpret_cast<V*>(Xh + row * xs + c * E) = v[u];
          }
        }
      } else {
        const unsigned magic = (1u << 20) / (unsigned)wp + 1u;
        for (int t = i; t < (k + 1) * wp; t += NP) {
          const int row = (int)(((unsigned)t * magic) >> 20);
          const int c = t - row * wp;
          Xh[row * xs + c] = c < w ? ((row < k ? feat_nn : feat_q) + idxh[row] + d0)[c] : T(0);
        }
      }
      if (aniso)
        for (int c = lane; c < wp; c += 64) ilbuf[c] = c < w ? T(1) / ls[d0 + c] : T(0);
      __syncthreads();
      if (i < k) {
        const T* xo = Xh + i * xs;
        const T* xq = Xh + k * xs;
        for (int c0 = 0; c0 < wp; c0 += E) {
          V df = *reinterpret_cast<const V*>(xq + c0) - *reinterpret_cast<const V*>(xo + c0);
          if (aniso) df = df * *reinterpret_cast<const V*>(ilbuf + c0);
#pragma unroll
          for (int e = 0; e < E; ++e) acc += df[e] * df[e];
        }
      }
    }
    // (all 64 lanes: acc = 0 where i >= k, and the evaluator does not look at it there)
    const T x = metric_arg<T>(acc, a.metric_id, post_scale);
    T kv;
    if constexpr (sizeof(T) == 4) kv = matern_gen_eval_group<NP>(x, i < k, gtab, (float)nu, g.h, g.lc);
    else kv = matern_gen_batch64_group<NP>(x, i < k, gtab, nu, g.h64, g.lc64, g.xmin64);
    for (int r = 0; r < R; ++r) {
      T part = i < k ? kv * coeffs[(crow * k + i) * (int64_t)R + r] : T(0);
#pragma unroll
      for (int off = NP / 2; off > 0; off >>= 1) part += __shfl_xor(part, off, 64);
      if (live && i == 0) mean[nb * R + r] = part;
    }
  }
}

// the name and geometry the library remembers of a general-smoothness prediction launch (mgp_last_kernel_name)
template <typename T>
static void note_fast_gen(const char* kernel, int np, int64_t grid, size_t lds) {
  if (np) note_launch("mgp::%s<%s, %d>", kernel, sizeof(T) == 4 ? "float" : "double", np);
  else note_launch("mgp::%s<%s>", kernel, sizeof(T) == 4 ? "float" : "double");
  note_launch_geometry(grid, lds);
}

template <typename T, int NP>
static int launch_fast_gen_np(FastArgs a, double nu, hipStream_t stream) {
  constexpr int NH = 64 / NP;
  constexpr int E = fv16<T>::N;
  constexpr int CH = 2 * E;
  const int dpad = (a.d + CH - 1) / CH * CH;
  a.dst = dpad < 64 ? dpad : 64;
  a.xs = a.dst + E;
  const uintptr_t align = (uintptr_t)a.feat_q | (uintptr_t)a.feat_nn;
  a.vec_ok = (a.d % E == 0) && (align % 16 == 0);
  size_t lds = ((size_t)NH * NP * a.xs + a.dst + (a.dst & 1)) * sizeof(T) + 64 * sizeof(int64_t);
  lds = (lds + 15) & ~(size_t)15;
  GenLaunch g = gen_launch_constants(nu, sizeof(T) == 8);
  g.tab = (int)lds;  // the node table: behind everything else (fp64, 64 features: 35 + 4 KiB)
  lds += gen_table_bytes(sizeof(T));
  const int64_t ntasks = (a.b + NH - 1) / NH;
  int64_t grid = kAssumedCus * 16;  // memory-bound: grid-stride over plenty of resident waves
  if (grid > ntasks) grid = ntasks;
  hipLaunchKernelGGL((fast_mean_gen_kernel<T, NP>), dim3((unsigned)grid), dim3(64), lds, stream, a, g, nu);
  MGP_HIP_CHECK_LAUNCH();
  note_fast_gen<T>("fast_mean_gen_kernel", NP, grid, lds);
  return MGP_OK;
}

// fast_mean_wide_kernel with the covariances from the node table: the last feature chunk leaves the squared distances
// in kv[], then the wave turns them into covariances in whole evaluator calls (4 / 2 neighbours per lane and call, lane
// i owns neighbours i, i + 64, ... as in the passes; neighbours past k are dead in `live`), and the sums follow as
// before.  One test point per wave: the wave's node count is the point's own.
// dynamic LDS carve: fast_mean_wide_kernel's, + the node table at byte g.tab behind it
template <typename T>
__global__ __launch_bounds__(64) void fast_mean_wide_gen_kernel(FastArgs a, GenLaunch g, double nu) {
  constexpr int E = fv16<T>::N;
  constexpr int CH = 2 * E;
  constexpr int PC = gen_pairs_per_call<T>();
  using V = typename fv16<T>::type;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int k = a.k, d = a.d, R = a.R, xs = a.xs, dst = a.dst;
  const int npass = (k + 63) / 64;
  int64_t* idxbuf = reinterpret_cast<int64_t*>(smem);
  T* tile = reinterpret_cast<T*>(idxbuf + 64);
  T* xq = tile + 64 * xs;
  T* ilbuf = tile + 65 * xs;
  T* kv = ilbuf + dst;
  const T* gtab = reinterpret_cast<const T*>(smem + g.tab);

  const T* feat_q = static_cast<const T*>(a.feat_q);
  const T* feat_nn = static_cast<const T*>(a.feat_nn);
  const T* coeffs = static_cast<const T*>(a.coeffs);
  const T* ls = static_cast<const T*>(a.length_scale);
  T* mean = static_cast<T*>(a.mean);
  const bool aniso = a.ls_count > 1;
  T post_scale = T(1);
  if (!aniso) {
    const T l = ls[0];
    post_scale = a.metric_id == MGP_METRIC_L2 ? T(1) / l : T(1) / (l * l);
  }
  const int lane = threadIdx.x;
  gen_build_node_table<T>(reinterpret_cast<T*>(smem + g.tab), nu, g, lane);  // (visible behind the point loop's barriers)

  for (int64_t nb = blockIdx.x; nb < a.b; nb += gridDim.x) {
    const int64_t* nrow = a.nn_idx + nb * k;
    const T* qrow = feat_q + (a.batch_idx ? a.batch_idx[nb] : nb) * (int64_t)d;
    const int64_t crow = a.coeff_row[nb];
    for (int d0 = 0; d0 < d; d0 += dst) {
      const int w = min(dst, d - d0);
      const int wp = (w + CH - 1) / CH * CH;
      __syncthreads();  // the tile's and kv's readers of the chunk / the test point before are done
      if (a.vec_ok) {
        if (lane < wp / E) *reinterpret_cast<V*>(xq + lane * E) = lane < w / E ? *reinterpret_cast<const V*>(qrow + d0 + lane * E) : V(0);
      } else {
        for (int c = lane; c < wp; c += 64) xq[c] = c < w ? qrow[d0 + c] : T(0);
      }
      if (aniso)
        for (int c = lane; c < wp; c += 64) ilbuf[c] = c < w ? T(1) / ls[d0 + c] : T(0);
      for (int p = 0; p < npass; ++p) {
        const int i = p * 64 + lane;
        const int nrows = min(64, k - p * 64);
        if (p > 0) __syncthreads();  // the pass before has read its rows
        idxbuf[lane] = i < k ? nrow[i] * (int64_t)d : 0;
        __syncthreads();
        if (a.vec_ok) {
          const int c16 = w / E, c16p = wp / E;
          const int rpr = 64 / c16p;
          const int sub = (int)(((unsigned)lane * ((1u << 16) / (unsigned)c16p + 1u)) >> 16);
          const int c = lane - sub * c16p;
          const bool lane_on = sub < rpr;
          constexpr int U = 6;
          for (int r0 = 0; r0 < nrows; r0 += U * rpr) {
            V v[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
              const int row = r0 + u * rpr + sub;
              v[u] = V(0);
              if (lane_on && row < nrows && c < c16) v[u] = *reinterpret_cast<const V*>(feat_nn + idxbuf[row] + d0 + c * E);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
              const int row = r0 + u * rpr + sub;
              if (lane_on && row < nrows) *reinterpret_cast<V*>(tile + row * xs + c * E) = v[u];
            }
          }
        } else {
          const unsigned magic = (1u << 20) / (unsigned)wp + 1u;
          for (int t = lane; t < nrows * wp; t += 64) {
            const int row = (int)(((unsigned)t * magic) >> 20);
            const int c = t - row * wp;
            tile[row * xs + c] = c < w ? (feat_nn + idxbuf[row] + d0)[c] : T(0);
          }
        }
        __syncthreads();
        if (i < k) {
          const T* xo = tile + lane * xs;
          T acc = d0 > 0 ? kv[i] : T(0);
          for (int c0 = 0; c0 < wp; c0 += E) {
            V df = *reinterpret_cast<const V*>(xq + c0) - *reinterpret_cast<const V*>(xo + c0);
            if (aniso) df = df * *reinterpret_cast<const V*>(ilbuf + c0);
#pragma unroll
            for (int e = 0; e < E; ++e) acc += df[e] * df[e];
          }
          kv[i] = acc;  // (the squared distance: the covariances are a phase of their own below)
        }
      }
    }
    // squared distances -> covariances, each by the lane that wrote it (a uniform trip count: every lane in every call)
    for (int i0 = 0; i0 < k; i0 += 64 * PC) {
      T v[PC];
      unsigned lv = 0;
#pragma unroll
      for (int u = 0; u < PC; ++u) {
        const int i = i0 + u * 64 + lane;
        v[u] = T(1);
        if (i < k) {
          v[u] = metric_arg<T>(kv[i], a.metric_id, post_scale);
          lv |= 1u << u;
        }
      }
      if constexpr (sizeof(T) == 4) matern_gen_eval<PC>(v, lv, gtab, (float)nu, g.h, g.lc);
      else matern_gen_batch64<PC>(v, lv, gtab, nu, g.h64, g.lc64, g.xmin64);
#pragma unroll
      for (int u = 0; u < PC; ++u)
        if ((lv >> u) & 1u) kv[i0 + u * 64 + lane] = v[u];
    }
    __syncthreads();
    const T* co = coeffs + crow * (int64_t)k * R;
    for (int r = 0; r < R; ++r) {
      T part = T(0);
      for (int i = lane; i < k; i += 64) part += kv[i] * co[i * (int64_t)R + r];
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) part += __shfl_xor(part, off, 64);
      if (lane == 0) mean[nb * R + r] = part;
    }
  }
}

template <typename T>
static int launch_fast_wide_gen(FastArgs a, double nu, hipStream_t stream) {
  constexpr int E = fv16<T>::N;
  constexpr int CH = 2 * E;
  const int dpad = (a.d + CH - 1) / CH * CH;
  a.dst = dpad < 64 ? dpad : 64;
  a.xs = a.dst + E;
  const uintptr_t align = (uintptr_t)a.feat_q | (uintptr_t)a.feat_nn;
  a.vec_ok = (a.d % E == 0) && (align % 16 == 0);
  // (fast_mean_wide_kernel's carve: at most 44 KiB; with the fp64 node table 48 KiB, inside the default limit)
  size_t lds = 64 * sizeof(int64_t) + ((size_t)65 * a.xs + a.dst + (size_t)(a.k + 63) / 64 * 64) * sizeof(T);
  lds = (lds + 15) & ~(size_t)15;
  GenLaunch g = gen_launch_constants(nu, sizeof(T) == 8);
  g.tab = (int)lds;
  lds += gen_table_bytes(sizeof(T));
  int64_t grid = kAssumedCus * 16;  // memory-bound: grid-stride over plenty of resident waves
  if (grid > a.b) grid = a.b;
  hipLaunchKernelGGL((fast_mean_wide_gen_kernel<T>), dim3((unsigned)grid), dim3(64), lds, stream, a, g, nu);
  MGP_HIP_CHECK_LAUNCH();
  note_fast_gen<T>("fast_mean_wide_gen_kernel", 0, grid, lds);
  return MGP_OK;
}

// mgp_fast_posterior_mean_gen_*: the dispatch of launch_fast_mean (a.kernel_id is not read)
template <typename T>
int launch_fast_mean_gen(const void* fq, const void* fn, int d, const int64_t* bi, const int64_t* ni, int64_t b, int k,
                         const void* coeffs, const int64_t* crow, int R, double smoothness, int metric_id, const void* ls,
                         int ls_count, void* mean, hipStream_t stream) {
  FastArgs a{fq, fn, bi, ni, coeffs, crow, ls, mean, b, d, k, R, MGP_KERNEL_MATERN_GEN, metric_id, ls_count, 0, 0, 0};
  if (k + 1 <= 32) return launch_fast_gen_np<T, 32>(a, smoothness, stream);
  if (k + 1 <= 64) return launch_fast_gen_np<T, 64>(a, smoothness, stream);
  return launch_fast_wide_gen<T>(a, smoothness, stream);
}

template int launch_fast_mean_gen<float>(const void*, const void*, int, const int64_t*, const int64_t*, int64_t, int,
                                         const void*, const int64_t*, int, double, int, const void*, int, void*, hipStream_t);
template int launch_fast_mean_gen<double>(const void*, const void*, int, const int64_t*, const int64_t*, int64_t, int,
                                          const void*, const int64_t*, int, double, int, const void*, int, void*, hipStream_t);

template <typename T>
int launch_fast_mean(const void* fq, const void* fn, int d, const int64_t* bi, const int64_t* ni, int64_t b, int k,
                     const void* coeffs, const int64_t* crow, int R, int kernel_id, int metric_id, const void* ls,
                     int ls_count, void* mean, hipStream_t stream) {
  FastArgs a{fq, fn, bi, ni, coeffs, crow, ls, mean, b, d, k, R, kernel_id, metric_id, ls_count, 0, 0, 0};
  if (k + 1 <= 32) return launch_fast_np<T, 32>(a, stream);
  if (k + 1 <= 64) return launch_fast_np<T, 64>(a, stream);
  return launch_fast_wide<T>(a, stream);
}

template int launch_fast_mean<float>(const void*, const void*, int, const int64_t*, const int64_t*, int64_t, int,
                                     const void*, const int64_t*, int, int, int, const void*, int, void*, hipStream_t);
template int launch_fast_mean<double>(const void*, const void*, int, const int64_t*, const int64_t*, int64_t, int,
                                      const void*, const int64_t*, int, int, int, const void*, int, void*, hipStream_t);

}  // namespace mgp
