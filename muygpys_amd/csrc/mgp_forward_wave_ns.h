// Posterior forward at wave size with a length scale per neighbourhood (mgp_posterior_ns_wave_*): k + 1 + R <= 64 slots,
// Isotropy, mean / variance / y^T K^-1 y of NH = 64 / NP neighbourhoods per wavefront, each with its own scale.
//
// A kernel of its own, in translation units of its own (mgp_forward_wave_ns.hip, mgp_forward_wave_ns_f32.hip): the
// headline fused_wave_kernel cannot take a scale per neighbourhood without moving its register allocation, and this is
// not ns_wave_backward_kernel with parts removed either.  What a forward allows that the backward does not:
//
//   * The feature tile is needed for the distances alone.  Behind the barrier that ends task t's distance phase the
//     gather of task t + 1 is requested into the SAME tile by LDS DMA (glds16_asm_at: no registers, invisible to the
//     compiler's wait counts) and lands under task t's covariances and elimination; task t + 1 starts with
//     lds_dma_wait().  Pad columns and unused slot rows are zeroed once, in front of the task loop: the DMA writes live
//     rows x the row's 16-byte groups only.  Index, nugget, first response and scale of task t + 1 are in registers one
//     task ahead (requested in two steps around task t's distance phase: the index first, what it addresses behind it).
//   * No multiplier is stored and nothing is substituted back: the responses ride along as R more rows of the
//     augmented system (row k + 1 + r = [y_r | 0]), and after the k elimination steps the outputs are Schur entries,
//         var = A_k[k],   mean_r = -A_{k+1+r}[k],   y_r^T K^-1 y_r = -A_{k+1+r}[k+1+r].
//   * The broadcast column of an elimination step alternates between two buffers: one barrier per step, not two.
//   * 1 / l stays in a register (one value per lane, the scale of the lane's half): the record shows no spill.
//
// FusedArgs::length_scale is not read.  A scale that is not finite and > 0: the half computes at l = 1 (no NaN reaches a
// pivot test) and stores NaN in its mean / var / ykinvy rows with one count in info, as for a non-positive pivot; a
// neighbourhood with both counts once.  The units are compiled with the packed fp32 instructions switched off and
// contain no hand-written ones.
#pragma once
#include "mgp_assemble.h"  // NsLaunch
#include "mgp_wave_common.h"

namespace mgp {

// DG: 16-byte groups of a (zero-padded) feature row
template <typename T, int NP, int DG>
__global__ __launch_bounds__(64, (sizeof(T) == 8 && NP == 64) ? 1 : 2) void ns_wave_forward_kernel(FusedArgs a, int vec_ok, NsLaunch n) {
  constexpr int NH = 64 / NP;
  // the cyclic BA x BP pair scheme of the wave backwards: lane i owns the pairs (i + own_offset(j), i + s)
  constexpr int NS = NP / 2, BA = 4, BP = NS / BA;
  auto own_offset = [](int j) { return j == 0 ? 0 : (j + 1) * BP + 1; };
  constexpr int E = v16<T>::N, CH = 2 * E, KS = NP + E;
  constexpr int SPR = DG + 1;     // 16-byte slots per tile row, the last one padding (an odd count)
  constexpr int xs = SPR * E;
  constexpr int wp = DG * E;      // padded feature count
  static_assert(wp % CH == 0, "DG must be even");
  using V = typename v16<T>::type;
  using ACC = typename v16<T>::acc;
  const int k = a.k, d = a.d, R = a.R;

  extern __shared__ __attribute__((aligned(16))) char smem[];
  T* X = reinterpret_cast<T*>(smem);  // 64 rows x xs: the tile starts the dynamic LDS (the DMA's base)
  T* M = X + 64 * xs;                 // NH x NP x KS: exchange matrix
  T* colbuf = M + 64 * KS;            // 2 x 64: the broadcast column, alternating
  int64_t* idxbuf = reinterpret_cast<int64_t*>(colbuf + 128);  // 64 row offsets (elements)

  const T* lsb = static_cast<const T*>(n.ls_batch);
  const T* feat_q = static_cast<const T*>(a.feat_q);
  const T* feat_nn = static_cast<const T*>(a.feat_nn);
  const T* targets = static_cast<const T*>(a.targets);
  const T* noise_dev = static_cast<const T*>(a.noise_dev);
  T* mean = static_cast<T*>(a.mean);
  T* var = static_cast<T*>(a.var);
  T* ykp = static_cast<T*>(a.ykinvy);
  const bool l2 = a.metric_id == MGP_METRIC_L2;
  const int dv = (d + E - 1) / E;
  const int64_t ntasks = (a.b + NH - 1) / NH;

  // ---- phase 0, one task ahead ------------------------------------------------------------------------------------
  // (a dead half of the odd tail reads the first neighbourhood of its task: valid rows, nothing of it is stored)
  auto nbb_of = [&](int64_t task, int h) {
    const int64_t nb = task * NH + h;
    return nb < a.b ? nb : task * NH;
  };
  int64_t nidx = 0;
  T neps = T(0), ny0 = T(0), nl = T(1);
  auto fetch_head = [&](int64_t task, int lane) {  // the index and the scale
    const int h = NH == 1 ? 0 : lane / NP, i = lane & (NP - 1);
    const int64_t nbb = nbb_of(task, h);
    nl = lsb[nbb];
    nidx = 0;
    if (i < k) nidx = a.nn_idx[nbb * k + i];
    else if (i == k) nidx = a.batch_idx ? a.batch_idx[nbb] : nbb;
  };
  auto fetch_tail = [&](int64_t task, int lane) {  // what the index addresses: nugget, first response, the feature rows
    const int h = NH == 1 ? 0 : lane / NP, i = lane & (NP - 1);
    const int64_t nbb = nbb_of(task, h);
    neps = T(0), ny0 = T(0);
    if (i < k) {
      if (a.noise_mode == MGP_NOISE_SCALAR) neps = (T)a.noise_scalar;
      else if (a.noise_mode == MGP_NOISE_TABLE) neps = noise_dev[nidx];
      else neps = noise_dev[nbb * k + i];
      ny0 = targets[(a.targets_batch ? nbb * k + i : nidx) * (int64_t)R];
    }
    idxbuf[lane] = nidx * (int64_t)d;
    __syncthreads();
    if (vec_ok) {
      // ---- phase 1: 16-byte slot sigma = 64 u + lane of the tile is (row, column) = (sigma / SPR, sigma % SPR);
      // piece u fills 64 consecutive slots.  Lanes on a pad column, a column past the row or a slot without a row
      // are switched off: those cells keep the zeros written in front of the task loop.
      unsigned tile = lds_byte_address(smem);
      asm volatile("" : "+s"(tile));  // (opaque: one base register, a scalar add per piece)
#pragma unroll
      for (int u = 0; u < SPR; ++u) {
        const int sigma = 64 * u + lane;
        const int row = sigma / SPR, c = sigma - row * SPR;
        const int slot = row & (NP - 1);
        if (slot <= k && c < dv) glds16_asm_at((slot < k ? feat_nn : feat_q) + idxbuf[row] + c * E, tile + u * 1024);
      }
    }
  };

  // pad columns and unused slot rows: zero, once (complete before the first transfer is requested)
  for (int t = threadIdx.x; t < 64 * SPR; t += 64) *reinterpret_cast<V*>(X + t * E) = V(0);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __syncthreads();
  if ((int64_t)blockIdx.x < ntasks) {
    fetch_head(blockIdx.x, threadIdx.x);
    fetch_tail(blockIdx.x, threadIdx.x);
  }

  for (int64_t task = blockIdx.x; task < ntasks; task += gridDim.x) {
    lds_dma_wait();  // this task's tile (requested during the previous task) has landed
    __syncthreads();
    // (opaque per task: as loop invariants the lane's row addresses of every phase are hoisted in front of the task loop
    // and spilled -- 400 to 800 registers in the fp32 forms)
    int lane = threadIdx.x;
    asm volatile("" : "+v"(lane));
    const int h = NH == 1 ? 0 : lane / NP;
    const int i = lane & (NP - 1);
    const T* Xh = X + h * NP * xs;
    T* Mh = M + h * NP * KS;
    const int64_t nb = task * NH + h;
    const bool live = nb < a.b;
    const int64_t nbb = live ? nb : task * NH;
    const int64_t myidx = nidx;
    const T myeps = neps, myy0 = ny0;
    const bool bad_scale = !(nl > T(0) && nl < num<T>::inf());
    const T inv_l = T(1) / (bad_scale ? T(1) : nl);

    if (!vec_ok) {  // rows that are not whole aligned 16-byte groups: element-wise with a masked tail, no overlap
      for (int t = lane; t < 64 * DG; t += 64) {
        const int row = t / DG, c = t - row * DG;
        const int slot = row & (NP - 1);
        if (slot <= k && c < dv) {
          const T* src = (slot < k ? feat_nn : feat_q) + idxbuf[row] + c * E;
          V v = V(0);
#pragma unroll
          for (int e = 0; e < E; ++e)
            if (c * E + e < d) v[e] = src[e];
          *reinterpret_cast<V*>(X + row * xs + c * E) = v;
        }
      }
      __syncthreads();
    }
    const int64_t next = task + gridDim.x;
    const bool more = next < ntasks;  // (uniform)
    if (more) fetch_head(next, lane);

    // the response rows k + 1 + r = [y_r | 0], column i by lane i (no pair store touches them; the exchange matrix
    // has been free since the previous task read its rows)
    if (i < k) {
      const T* ty = targets + (a.targets_batch ? nbb * k + i : myidx) * (int64_t)R;
      Mh[(k + 1) * KS + i] = myy0;
      for (int r = 1; r < R; ++r) Mh[(k + 1 + r) * KS + i] = ty[r];
    } else {
      for (int r = 0; r < R; ++r) Mh[(k + 1 + r) * KS + i] = T(0);
    }

    // ---- phase 2: squared distances of the lane's NS pairs, unscaled, difference form ---------------------------------
    ACC acc[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) acc[s] = ACC(0);
    // (a rolled loop over the chunks the row really has: unrolled over all DG groups, the reads of every chunk are
    // hoisted and spill 70 to 580 registers from DG = 8 on; the tile's zero padding covers the last chunk's second group)
    const int wlive = (dv + 1) / 2 * CH;
#pragma unroll 1
    for (int c0 = 0; c0 < wlive; c0 += CH) {
      V own0[BA], own1[BA];
#pragma unroll
      for (int j = 0; j < BA; ++j) {
        const T* xj = Xh + ((i + own_offset(j)) & (NP - 1)) * xs + c0;
        own0[j] = *reinterpret_cast<const V*>(xj);
        own1[j] = *reinterpret_cast<const V*>(xj + E);
      }
#pragma unroll
      for (int s = 1; s <= BP; ++s) {
        const T* xo = Xh + ((i + s) & (NP - 1)) * xs + c0;
        const V o0 = *reinterpret_cast<const V*>(xo);
        const V o1 = *reinterpret_cast<const V*>(xo + E);
#pragma unroll
        for (int j = 0; j < BA; ++j) {
          accum(acc[j * BP + s - 1], own0[j] - o0);
          accum(acc[j * BP + s - 1], own1[j] - o1);
        }
      }
      __builtin_amdgcn_sched_barrier(0);  // (one chunk's reads in flight: all hoisted, they spill)
    }
    __syncthreads();  // every read of the tile is behind us: the next task's rows may land
    if (more) fetch_tail(next, lane);

    // ---- phase 3: covariances -> lower triangle of the exchange matrix -> row per lane --------------------------------
    // CB pairs at a time, each batch stored before the next is evaluated: the accumulators die batch by batch (all NS
    // covariances in flight at once cost the fp64 forms 130 spilled registers)
    {
      constexpr int CB = 4;
      static_assert(NS % CB == 0, "whole batches");
      const T post_scale = l2 ? inv_l : inv_l * inv_l;
      const int dump = (NP - 1) * KS + NP;  // padding behind the last row
      kernel_dispatch(a.kernel_id, a.metric_id, [&](auto kid, auto mid) {
        constexpr int KID = decltype(kid)::value, MID = decltype(mid)::value;
#pragma unroll
        for (int s0 = 0; s0 < NS; s0 += CB) {
          T kv[CB];
          if constexpr (sizeof(T) == 4) {
#pragma unroll
            for (int u = 0; u < CB; u += 2) {
              const f2 kk = cov_from_sqdist2(f2{acc_total(acc[s0 + u]), acc_total(acc[s0 + u + 1])}, KID, MID, post_scale);
              kv[u] = kk.x;
              kv[u + 1] = kk.y;
            }
          } else {
#pragma unroll
            for (int u = 0; u < CB; ++u) kv[u] = acc_total(acc[s0 + u]);
            cov_batch64<CB, KID, MID>(kv, post_scale);  // (stage by stage: CB dependent chains interleaved)
          }
#pragma unroll
          for (int u = 0; u < CB; ++u) {
            const int s = s0 + u;
            const int r1 = (i + own_offset(s / BP)) & (NP - 1);
            const int c = (i + s % BP + 1) & (NP - 1);
            const int hi = max(r1, c), lo = min(r1, c);
            // rows <= k: neighbour x neighbour, or neighbour x query (lo < hi <= k); a pair with a slot behind them is dropped
            Mh[hi <= k ? hi * KS + lo : dump] = kv[u];
          }
          __builtin_amdgcn_sched_barrier(0);
        }
      });
      if (i <= k) Mh[i * KS + i] = i < k ? T(1) + myeps : T(1);  // (a response row's diagonal is among its zeros)
    }
    __syncthreads();
    V A[NP / E];
#pragma unroll
    for (int c4 = 0; c4 < NP / E; ++c4)
      A[c4] = i <= k + R ? *reinterpret_cast<const V*>(Mh + i * KS + c4 * E) : V(0);  // slots behind the responses: zero rows

    // ---- phase 4: elimination, steps j < k; no multiplier is kept ------------------------------------------------------
    __builtin_amdgcn_s_setprio(2);  // chains of short dependent steps go first
    bool bad = false;
#pragma unroll
    for (int j = 0; j < NP - 2; ++j) {  // (k + 1 + R <= NP: k <= NP - 2)
      if (j < k) {  // (uniform)
        T* colh = colbuf + (j & 1) * 64 + h * NP;
        const T ajj = A[j / E][j % E];
        colh[i] = ajj;
        __syncthreads();
        const V cp = *reinterpret_cast<const V*>(colh + (j / E) * E);
        const T p = cp[j % E];
        bad = bad || !(p > T(0));
        const T t = ajj * pivot_rcp(p);
        const V nt = V(-t);
        A[j / E] = cp * nt + A[j / E];
        constexpr int GC = sizeof(T) == 4 ? 8 : 4;
#pragma unroll
        for (int c0 = j / E + 1; c0 < NP / E; c0 += GC) {
          V cv[GC];
#pragma unroll
          for (int u = 0; u < GC; ++u)
            if (c0 + u < NP / E) cv[u] = *reinterpret_cast<const V*>(colh + (c0 + u) * E);
#pragma unroll
          for (int u = 0; u < GC; ++u)
            if (c0 + u < NP / E) A[c0 + u] = cv[u] * nt + A[c0 + u];
        }
        // The last step (uniform): the rows k .. k + R park their columns >= k in the exchange matrix, free since the
        // rows were read.  Inside the step, so that no register of the row lives past the loop: read behind it, the
        // row is a value merged from every step's exit, which cost the fp32 forms 400 to 700 spilled registers.
        if (j + 1 == k && i >= k && i <= k + R) {
#pragma unroll
          for (int c4 = (j + 1) / E; c4 < NP / E; ++c4) *reinterpret_cast<V*>(Mh + i * KS + c4 * E) = A[c4];
        }
      }
    }
    __builtin_amdgcn_s_setprio(0);

    // ---- phase 5: the outputs are Schur entries of the rows k .. k + R, read through LDS -------------------------------
    // (k is a run-time value: a run-time index into the register row would go to scratch)
    const bool response = i > k && i <= k + R;
    __syncthreads();
    if (live) {
      const bool fail = bad || bad_scale;
      if (i == k) var[nb] = fail ? num<T>::nan() : Mh[k * KS + k];
      if (response) {
        const int64_t o = nb * R + (i - k - 1);
        mean[o] = fail ? num<T>::nan() : -Mh[i * KS + k];
        if (ykp) ykp[o] = fail ? num<T>::nan() : -Mh[i * KS + i];
      }
      if (fail && i == 0 && a.info) atomicAdd(a.info, 1);
    }
  }
}

// LDS carve, vector eligibility and the resident grid of one instantiation
template <typename T, int NP, int DG>
static int launch_fwd_ns_np(const FusedArgs& a, const void* ls_batch, hipStream_t stream) {
  constexpr int NH = 64 / NP;
  constexpr int E = v16<T>::N, KS = NP + E, xs = DG * E + E;
  const uintptr_t align = (uintptr_t)a.feat_q | (uintptr_t)a.feat_nn;
  const int vec_ok = (a.d % E == 0) && (align % 16 == 0);
  const size_t lds = ((size_t)64 * xs + (size_t)64 * KS + 2 * 64) * sizeof(T) + 64 * sizeof(int64_t);
  static Residency res;
  const LaunchLabel label(a.b, a.k, a.d, a.R, "mgp::ns_wave_forward_kernel<%s,%d,%d>", sizeof(T) == 4 ? "float" : "double", NP, DG);
  return launch_resident(&ns_wave_forward_kernel<T, NP, DG>, res, 64, lds, (a.b + NH - 1) / NH, nullptr, stream, &label, a, vec_ok,
                         NsLaunch{ls_batch}).status;
}

// by the row's 16-byte groups
template <typename T, int NP>
int launch_fwd_ns_dg(const FusedArgs& a, const void* ls_batch, hipStream_t stream) {
  constexpr int E = v16<T>::N;
  const int dv = (a.d + E - 1) / E;
  if (dv <= 4) return launch_fwd_ns_np<T, NP, 4>(a, ls_batch, stream);
  if (dv <= 8) return launch_fwd_ns_np<T, NP, 8>(a, ls_batch, stream);
  if constexpr (sizeof(T) == 8) {
    return MGP_EUNSUPPORTED;
  } else {
    if (dv <= 10) return launch_fwd_ns_np<T, NP, 10>(a, ls_batch, stream);
    if (dv <= 12) return launch_fwd_ns_np<T, NP, 12>(a, ls_batch, stream);
    return launch_fwd_ns_np<T, NP, 16>(a, ls_batch, stream);
  }
}

}  // namespace mgp
