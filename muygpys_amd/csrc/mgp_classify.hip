// Classification on the device (the reference's _src/optimize/loss/numpy.py:12-19 and
// examples/classify.py:537-607 / examples/two_class_classify_uq.py:346-423):
//   * class_sums_kernel: the loss sums of a (b, R) prediction against one-hot targets -- cross-entropy, mse,
//     pseudo-Huber, the argmax agreement -- and, optionally, the cotangent of the chosen loss, one row per lane,
//     reduced in fp64 by a fixed two-stage tree (mgp_class_sums_*)
//   * class_flags_kernel / class_scan_kernel / class_compact_kernel: which neighbourhoods carry more than one
//     label, and the compacted list of those the solve still needs (mgp_class_partition_*)
//   * class_scatter_kernel: the solved rows back into the full prediction (mgp_class_scatter_*)
// No kernel here waits on another workgroup: kernel boundaries are the only synchronisation.
#include <cfloat>
#include <cmath>

#include "mgp_args.h"

namespace mgp {

static const int kClassBlock = 256;
static const int kClassBlocks = 1024;  // workgroups of a reduction / chunks of a partition: 6 doubles each fit the scratch

template <typename T> struct class_eps;
template <> struct class_eps<float> { static constexpr double value = FLT_EPSILON; };
template <> struct class_eps<double> { static constexpr double value = DBL_EPSILON; };

// every workgroup stores its six sums; class_reduce_kernel adds them in workgroup order
__device__ inline void class_block_store(double (&v)[6], double* scratch) {
  __shared__ double red[6][kClassBlock / MGP_WAVE];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    const double s = wave_sum(v[i]);
    if (lane == 0) red[i][w] = s;
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    double s = 0;
    for (int j = 0; j < kClassBlock / MGP_WAVE; ++j) s += red[threadIdx.x][j];
    scratch[(size_t)blockIdx.x * 6 + threadIdx.x] = s;
  }
}

__global__ void class_reduce_kernel(const double* scratch, int blocks, double* out) {
  __shared__ double red[kClassBlock];
  for (int i = 0; i < 6; ++i) {
    double s = 0;
    for (int b = threadIdx.x; b < blocks; b += kClassBlock) s += scratch[(size_t)b * 6 + i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int off = kClassBlock / 2; off > 0; off >>= 1) {
      if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
      __syncthreads();
    }
    if (threadIdx.x == 0) out[i] = red[0];
    __syncthreads();
  }
}

// One row per lane, R a run-time loop.  Row term of the cross-entropy (loss/numpy.py:12-19 with sklearn's
// log_loss(normalize=False) written out): one_hot = target > 0, p = softmax(row) (max-subtracted, fp64),
// -sum_c one_hot_c log(clip(p_c, eps, 1 - eps)), eps the machine epsilon of T.  Its cotangent:
// grad_j = sum_{c in one_hot, p_c not clipped} (p_j - delta_cj) = |A| p_j - [j in A].
template <typename T>
__global__ void class_sums_kernel(const T* __restrict__ pred, const char* __restrict__ target, int64_t tstride,
                                  const int64_t* __restrict__ batch_idx, int64_t b, int R, int loss_id,
                                  double grad_scale, double hd, T* __restrict__ grad_pred, double* scratch) {
  // (the loops over the classes stay rolled scalar loops: vectorised for float loads they doubled the body and the
  // constants of its fp64 exp left the scalar register file)
  constexpr double eps = class_eps<T>::value;
  double acc[6] = {0, 0, 0, 0, 0, 0};
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < b; i += (int64_t)gridDim.x * blockDim.x) {
    const T* x = pred + i * R;
    const T* y = reinterpret_cast<const T*>(target + (batch_idx ? batch_idx[i] : i) * tstride);
    double xmax = (double)x[0], ymax = (double)y[0];
    int xarg = 0, yarg = 0;
#pragma clang loop unroll(disable) vectorize(disable)
    for (int c = 1; c < R; ++c) {
      const double xc = (double)x[c], yc = (double)y[c];
      if (xc > xmax) xmax = xc, xarg = c;
      if (yc > ymax) ymax = yc, yarg = c;
    }
    double z = 0;
#pragma clang loop unroll(disable) vectorize(disable)
    for (int c = 0; c < R; ++c) z += ::exp((double)x[c] - xmax);
    // log p_c = x_c - max - log z: the clip to [eps, 1 - eps] is a clamp of the logarithm (no exp / log per class)
    const double logz = ::log(z), lo = ::log(eps), hi = ::log1p(-eps);
    double ce = 0, r2 = 0, hub = 0;
    int active = 0;  // |A|: one-hot classes whose probability the clip leaves alone
#pragma clang loop unroll(disable) vectorize(disable)
    for (int c = 0; c < R; ++c) {
      const double xc = (double)x[c], yc = (double)y[c];
      const double r = xc - yc;
      r2 += r * r;
      hub += hd * hd * (::sqrt(1.0 + (r / hd) * (r / hd)) - 1.0);
      if (yc > 0.0) {
        const double lp = xc - xmax - logz;
        const bool inside = lp >= lo && lp <= hi;
        ce -= inside ? lp : (lp < lo ? lo : hi);
        active += inside;
      }
    }
    acc[0] += ce;
    acc[1] += r2;
    acc[2] += (double)R;
    acc[3] += 1.0;
    acc[4] += xarg == yarg ? 1.0 : 0.0;
    acc[5] += hub;
    if (grad_pred) {
      T* g = grad_pred + i * R;
#pragma clang loop unroll(disable) vectorize(disable)
      for (int c = 0; c < R; ++c) {
        const double xc = (double)x[c], yc = (double)y[c];
        double v;
        if (loss_id == MGP_CLASS_LOSS_MSE) {
          v = 2.0 * (xc - yc);
        } else {
          const double lp = xc - xmax - logz;
          v = active * ::exp(lp) - ((yc > 0.0 && lp >= lo && lp <= hi) ? 1.0 : 0.0);
        }
        g[c] = (T)(grad_scale * v);
      }
    }
  }
  class_block_store(acc, scratch);
}

// ---- label agreement and compaction -------------------------------------------------------------------------------
// The rows are dealt to the workgroups in contiguous chunks, so workgroup order is row order and the compacted list
// comes out ascending.  A table index outside [0, n) is clamped into it (nothing is read out of bounds).

__device__ __forceinline__ int64_t class_row(int64_t idx, int64_t n) { return idx < 0 ? 0 : (idx >= n ? n - 1 : idx); }

// examples/classify.py:577-586: pred row = the first neighbour's labels; non-constant iff max != min of label
// COLUMN 0 over the k neighbours; counts[g] = non-constant rows of chunk g
template <typename T>
__global__ void class_flags_kernel(const T* __restrict__ labels, int64_t n, int R, const int64_t* __restrict__ nn_idx,
                                   int64_t b, int k, int64_t chunk, T* __restrict__ pred,
                                   unsigned char* __restrict__ nonconstant, int64_t* __restrict__ counts) {
  const int64_t lo = blockIdx.x * chunk, hi = lo + chunk < b ? lo + chunk : b;
  int total = 0;
  for (int64_t t0 = lo; t0 < hi; t0 += kClassBlock) {  // (uniform trip count: every lane reaches the barrier)
    const int64_t i = t0 + threadIdx.x;
    int flag = 0;
    if (i < hi) {
      const int64_t* ni = nn_idx + i * k;
      const int64_t first = class_row(ni[0], n);
      T lmin = labels[first * R], lmax = lmin;
      for (int j = 1; j < k; ++j) {
        const T v = labels[class_row(ni[j], n) * R];
        lmin = v < lmin ? v : lmin;
        lmax = v > lmax ? v : lmax;
      }
      flag = lmax != lmin;
      nonconstant[i] = (unsigned char)flag;
      for (int c = 0; c < R; ++c) pred[i * R + c] = labels[first * R + c];
    }
    total += __syncthreads_count(flag);
  }
  if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

// exclusive scan of the chunk counts, in place (one workgroup); *m = the total
__global__ void class_scan_kernel(int64_t* counts, int chunks, int64_t* m) {
  __shared__ int64_t part[kClassBlock];
  const int per = (chunks + kClassBlock - 1) / kClassBlock;
  const int lo = threadIdx.x * per, hi = lo + per < chunks ? lo + per : chunks;
  int64_t s = 0;
  for (int g = lo; g < hi; ++g) s += counts[g];
  part[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    int64_t run = 0;
    for (int t = 0; t < kClassBlock; ++t) {
      const int64_t v = part[t];
      part[t] = run;
      run += v;
    }
    *m = run;
  }
  __syncthreads();
  int64_t run = part[threadIdx.x];
  for (int g = lo; g < hi; ++g) {
    const int64_t v = counts[g];
    counts[g] = run;
    run += v;
  }
}

// sel[pos] = row, nn_sel[pos, :] = nn_idx[row, :] for the non-constant rows, pos ascending with the row
__global__ void class_compact_kernel(const unsigned char* __restrict__ nonconstant, const int64_t* __restrict__ nn_idx,
                                     int64_t b, int k, int64_t chunk, const int64_t* __restrict__ offsets,
                                     int64_t* __restrict__ sel, int64_t* __restrict__ nn_sel) {
  __shared__ int wave_count[kClassBlock / MGP_WAVE];
  __shared__ int64_t dst[kClassBlock];
  const int64_t lo = blockIdx.x * chunk, hi = lo + chunk < b ? lo + chunk : b;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int64_t base = offsets[blockIdx.x];
  for (int64_t t0 = lo; t0 < hi; t0 += kClassBlock) {
    const int64_t i = t0 + threadIdx.x;
    const int flag = i < hi ? (int)nonconstant[i] : 0;
    const unsigned long long mask = __ballot(flag);
    if (lane == 0) wave_count[w] = __popcll(mask);
    __syncthreads();
    int before = __popcll(mask & ((1ull << lane) - 1ull)), tile = 0;
    for (int j = 0; j < kClassBlock / MGP_WAVE; ++j) {
      if (j < w) before += wave_count[j];
      tile += wave_count[j];
    }
    dst[threadIdx.x] = flag ? base + before : (int64_t)-1;
    if (flag) sel[base + before] = i;
    __syncthreads();
    const int rows = (int)(hi - t0 < kClassBlock ? hi - t0 : kClassBlock);
    for (int e = threadIdx.x; e < rows * k; e += kClassBlock) {  // (the tile's index rows, read side by side)
      const int r = e / k, j = e - r * k;
      const int64_t p = dst[r];
      if (p >= 0) nn_sel[p * k + j] = nn_idx[(t0 + r) * k + j];
    }
    base += tile;
    __syncthreads();
  }
}

// dst[sel[i], :] = src[i, :] (+ the variance column); a row index outside [0, b) is skipped
template <typename T>
__global__ void class_scatter_kernel(const T* __restrict__ src_mean, const T* __restrict__ src_var,
                                     const int64_t* __restrict__ sel, int64_t m, int64_t b, int R, T* __restrict__ dst_mean,
                                     T* __restrict__ dst_var) {
  const int64_t total = m * R;
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = t / R;
    const int c = (int)(t - i * R);
    const int64_t row = sel[i];
    if (row < 0 || row >= b) continue;
    dst_mean[row * R + c] = src_mean[t];
    if (c == 0 && src_var) dst_var[row] = src_var[i];
  }
}

static inline int class_grid(int64_t n) {
  const int64_t g = ceil_div(n, kClassBlock);
  return (int)(g < 1 ? 1 : (g > kClassBlocks ? kClassBlocks : g));
}

template <typename T>
int launch_class_sums(const T* pred, const void* target, int64_t tstride, const int64_t* batch_idx, int64_t b, int R,
                      int loss_id, double grad_scale, double hd, T* grad_pred, double* out, double* scratch, hipStream_t s) {
  if (R < 2 || R > kClassMaxR) return MGP_EUNSUPPORTED;
  if (b == 0) {
    const hipError_t e = hipMemsetAsync(out, 0, 6 * sizeof(double), s);
    return e == hipSuccess ? MGP_OK : -(1000 + (int)e);
  }
  const int g = class_grid(b);
  hipLaunchKernelGGL(class_sums_kernel<T>, dim3(g), dim3(kClassBlock), 0, s, pred, static_cast<const char*>(target), tstride,
                     batch_idx, b, R, loss_id, grad_scale, hd, grad_pred, scratch);
  MGP_HIP_CHECK_LAUNCH();
  hipLaunchKernelGGL(class_reduce_kernel, dim3(1), dim3(kClassBlock), 0, s, scratch, g, out);
  MGP_HIP_CHECK_LAUNCH();
  return MGP_OK;
}

template <typename T>
int launch_class_partition(const T* labels, int64_t n, int R, const int64_t* nn_idx, int64_t b, int k, T* pred,
                           unsigned char* nonconstant, int64_t* count, int64_t* sel, int64_t* nn_sel, void* scratch,
                           hipStream_t s) {
  if (b == 0) {
    const hipError_t e = hipMemsetAsync(count, 0, sizeof(int64_t), s);
    return e == hipSuccess ? MGP_OK : -(1000 + (int)e);
  }
  const int g = class_grid(b);
  const int64_t chunk = ceil_div(b, g);
  int64_t* counts = static_cast<int64_t*>(scratch);
  hipLaunchKernelGGL(class_flags_kernel<T>, dim3(g), dim3(kClassBlock), 0, s, labels, n, R, nn_idx, b, k, chunk, pred,
                     nonconstant, counts);
  MGP_HIP_CHECK_LAUNCH();
  hipLaunchKernelGGL(class_scan_kernel, dim3(1), dim3(kClassBlock), 0, s, counts, g, count);
  MGP_HIP_CHECK_LAUNCH();
  hipLaunchKernelGGL(class_compact_kernel, dim3(g), dim3(kClassBlock), 0, s, nonconstant, nn_idx, b, k, chunk, counts, sel,
                     nn_sel);
  MGP_HIP_CHECK_LAUNCH();
  return MGP_OK;
}

template <typename T>
int launch_class_scatter(const T* src_mean, const T* src_var, const int64_t* sel, int64_t m, int64_t b, int R, T* dst_mean,
                         T* dst_var, hipStream_t s) {
  if (m == 0) return MGP_OK;
  hipLaunchKernelGGL(class_scatter_kernel<T>, dim3(class_grid(m * R)), dim3(kClassBlock), 0, s, src_mean, src_var, sel, m, b,
                     R, dst_mean, dst_var);
  MGP_HIP_CHECK_LAUNCH();
  return MGP_OK;
}

#define MGP_INSTANTIATE_CLASS(T)                                                                                     \
  template int launch_class_sums<T>(const T*, const void*, int64_t, const int64_t*, int64_t, int, int, double, double, \
                                    T*, double*, double*, hipStream_t);                                              \
  template int launch_class_partition<T>(const T*, int64_t, int, const int64_t*, int64_t, int, T*, unsigned char*,   \
                                         int64_t*, int64_t*, int64_t*, void*, hipStream_t);                          \
  template int launch_class_scatter<T>(const T*, const T*, const int64_t*, int64_t, int64_t, int, T*, T*, hipStream_t);
MGP_INSTANTIATE_CLASS(float)
MGP_INSTANTIATE_CLASS(double)

}  // namespace mgp
