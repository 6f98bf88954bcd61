// Hyper-parameter backward at wave size with a length scale per neighbourhood (the first rung of
// mgp_hyper_backward_ns_*): k + 2 <= 64 slots, Isotropy, the partials d loss / d l_nb and d loss / d eps alone.
//
// A kernel of its own, in translation units of its own (mgp_backward_wave_ns.hip, mgp_backward_wave_ns_f32.hip), on the
// phases of backward_wave_kernel (mgp_backward_wave_kernel.h states the maths and the phases): gather -> cyclic
// register-blocked pair distances -> covariances -> exchange -> row-per-lane elimination -> back-substitution -> pair
// cotangents.  It is not an instantiation of that kernel's text: routing that kernel through a shared body moves the
// register allocation of every existing instantiation, which sits within a few registers of its cap.  What this one
// does not have: the feature sweep, the q matrix, a compile-time nn_count, the hand-written packed fp32 blocks
// (dist_block4, vsub) -- its units are compiled with the packed fp32 instructions switched off.
//
// One wavefront owns NH = 64 / NP neighbourhoods and each has its own scale, so 1 / l is a PER-LANE value, read in
// phase 0 from the scale of the lane's half (`lsb[nbb]`: the first neighbourhood's in a dead half of the odd tail).  It
// stays a vector value -- every use (covariances, dk_dacc, the final gls) is a per-lane VALU operand already, so a
// v_readlane per half would buy nothing but a select in front of every use -- but it does not stay in a register: each
// lane parks it in its own slot of ilb (64 slots, idle under Isotropy) and reads it back at the three places of use,
// because the fp64 forms sit at the register cap and two more live doubles spilled 38 to 40 registers.
// FusedArgs::length_scale is not read.  A scale that is not finite and > 0: the half computes at l = 1 (no NaN reaches
// a shuffle or a pivot test) and stores NaN in its grad_ls and grad_noise rows with one count in info.
#pragma once
#include "mgp_assemble.h"  // NsLaunch
#include "mgp_wave_common.h"

namespace mgp {

// DG: 16-byte groups of a (zero-padded) feature row, as in backward_wave_kernel
template <typename T, int NP, int DG>
__global__ __launch_bounds__(64, (sizeof(T) == 8 && NP == 64) ? 1 : 2) void ns_wave_backward_kernel(BackwardArgs g, int vec_ok, NsLaunch n) {
  constexpr int KFIX = 0;
  constexpr bool HYPER = true, PERNB = true;
  const T* lsb = static_cast<const T*>(n.ls_batch);
  constexpr int NH = 64 / NP;
  constexpr int NS = NP / 2, BA = 4, BP = NS / BA;
  auto own_offset = [](int j) { return j == 0 ? 0 : (j + 1) * BP + 1; };
  constexpr int E = v16<T>::N, CH = 2 * E, KS = NP + E;
  constexpr int xs = DG * E + E;  // odd number of 16-byte slots per tile row
  using V = typename v16<T>::type;
  using ACC = typename v16<T>::acc;
  const FusedArgs& a = g.f;
  const int k = KFIX > 0 ? KFIX : a.k, d = a.d, R = a.R;

  extern __shared__ __attribute__((aligned(16))) char smem[];
  T* X = reinterpret_cast<T*>(smem);             // NH * NP rows x xs
  T* M = X + NH * NP * xs;                       // NH x NP x KS: exchange matrix, multipliers, then q
  T* colbuf = M + NH * NP * KS;                  // 64
  T* avec = colbuf + 64;                         // 64
  T* wvec = avec + 64;                           // 64
  T* ilb = wvec + 64;                            // 64: inverse length scales (Anisotropy; zero past d)
  int64_t* idxbuf = reinterpret_cast<int64_t*>(ilb + 64);  // 64 row offsets (elements)

  const T* feat_q = static_cast<const T*>(a.feat_q);
  const T* feat_nn = static_cast<const T*>(a.feat_nn);
  const T* targets = static_cast<const T*>(a.targets);
  const T* noise_dev = static_cast<const T*>(a.noise_dev);
  const T* gmean = static_cast<const T*>(g.grad_mean);
  const T* gvar = static_cast<const T*>(g.grad_var);
  const T* gyk = static_cast<const T*>(g.grad_yk);  // (LOOCV, R = 1: the right-hand side is y, w = gm u below)
  T* gq = static_cast<T*>(g.grad_feat_q);
  T* gnn = static_cast<T*>(g.grad_feat_nn);
  T* gtg = static_cast<T*>(g.grad_targets);
  T* gls = static_cast<T*>(g.grad_ls);
  T* gnz = static_cast<T*>(g.grad_noise);
  const bool l2 = a.metric_id == MGP_METRIC_L2;
  const bool aniso = a.ls_count > 1;  // (PERNB: the launcher admits ls_count == 1 alone)
  T inv_l = T(1);  // (PERNB: not used)
  if constexpr (!PERNB) inv_l = aniso ? T(1) : T(1) / static_cast<const T*>(a.length_scale)[0];
  const T post_scale = l2 ? inv_l : inv_l * inv_l;
  // 1 / l and the metric's factor at a place of use: the launch's (registers), or the lane's own (its slot of ilb)
  auto inv_l_here = [&]() -> T {
    if constexpr (PERNB) return ilb[threadIdx.x];
    else return inv_l;
  };
  auto post_scale_here = [&]() -> T {
    if constexpr (PERNB) {
      const T v = ilb[threadIdx.x];
      return l2 ? v : v * v;
    } else {
      return post_scale;
    }
  };
  if (aniso) {
    const int f = threadIdx.x;
    ilb[f] = f < a.d ? T(1) / static_cast<const T*>(a.length_scale)[f] : T(0);
  }
  constexpr int wp = DG * E;                     // padded feature count (a multiple of the distance loop's chunk)
  static_assert(wp % CH == 0, "DG must be even");
  const int dv = (d + E - 1) / E;
  const int64_t ntasks = (a.b + NH - 1) / NH;

  for (int64_t task = blockIdx.x; task < ntasks; task += gridDim.x) {
    int lane = threadIdx.x;
    asm volatile("" : "+v"(lane));
    const int h = NH == 1 ? 0 : lane / NP;
    const int i = lane & (NP - 1);
    T* Xh = X + h * NP * xs;
    T* Mh = M + h * NP * KS;
    T* colh = colbuf + h * NP;
    const int64_t nb = task * NH + h;
    const bool live = nb < a.b;
    const int64_t nbb = live ? nb : task * NH;

    // ---- phase 0: indices, nugget, combined right-hand side -----------------------------------------
    bool bad_scale = false;
    if constexpr (PERNB) {
      const T l = lsb[nbb];
      bad_scale = !(l > T(0) && l < num<T>::inf());
      ilb[lane] = T(1) / (bad_scale ? T(1) : l);
    }
    int64_t myidx = 0;
    T myeps = T(0), myyt = T(0);
    if (i < k) {
      myidx = a.nn_idx[nbb * k + i];
      if (a.noise_mode == MGP_NOISE_SCALAR) myeps = (T)a.noise_scalar;
      else if (a.noise_mode == MGP_NOISE_TABLE) myeps = noise_dev[myidx];
      else myeps = noise_dev[nbb * k + i];
      if (gyk) {
        myyt = targets[(a.targets_batch ? nbb * k + i : myidx) * (int64_t)R];
      } else if (gmean) {
        const T* ty = targets + (a.targets_batch ? nbb * k + i : myidx) * (int64_t)R;
        for (int r = 0; r < R; ++r) myyt += gmean[nbb * R + r] * ty[r];
      }
    } else if (i == k) {
      myidx = a.batch_idx ? a.batch_idx[nbb] : nbb;
    }
    __syncthreads();
    idxbuf[lane] = myidx * (int64_t)d;
    __syncthreads();

    // ---- phase 1: feature tile (rows 0 .. k of each half; other slots zero rows) ---------------------
    {
      constexpr int c16p = DG;
      for (int t = lane; t < NH * NP * c16p; t += 64) {
        const int row = t / c16p, c = t - row * c16p;
        const int slot = row & (NP - 1);
        V v = V(0);
        if (slot <= k && c < dv) {
          const T* src = (slot < k ? feat_nn : feat_q) + idxbuf[row] + c * E;
          if (vec_ok) {
            v = *reinterpret_cast<const V*>(src);
          } else {
#pragma unroll
            for (int e = 0; e < E; ++e)
              if (c * E + e < d) v[e] = src[e];
          }
        }
        *reinterpret_cast<V*>(X + row * xs + c * E) = v;
      }
    }
    __syncthreads();
    if (aniso) {  // z = x / l, in place (slot rows only: the right-hand-side slot is a zero row)
      T* xrow = Xh + i * xs;
#pragma unroll
      for (int c4 = 0; c4 < DG; ++c4) {
        V x = *reinterpret_cast<const V*>(xrow + c4 * E);
        x = x * *reinterpret_cast<const V*>(ilb + c4 * E);
        *reinterpret_cast<V*>(xrow + c4 * E) = x;
      }
      __syncthreads();
    }

    // ---- phase 2: squared distances of the lane's NS pairs (kept: the derivative needs them) --------
    ACC acc[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) acc[s] = ACC(0);
#pragma unroll
    for (int c0 = 0; c0 < wp; c0 += CH) {
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
        if constexpr (sizeof(T) == 4 && BA == 4 && !PERNB) {
          // hand-ordered packed blocks: no instruction reads its predecessor's result (mgp_wave_common.h)
          dist_block4(acc[s - 1], acc[BP + s - 1], acc[2 * BP + s - 1], acc[3 * BP + s - 1], own0[0], own0[1], own0[2],
                      own0[3], o0);
          dist_block4(acc[s - 1], acc[BP + s - 1], acc[2 * BP + s - 1], acc[3 * BP + s - 1], own1[0], own1[1], own1[2],
                      own1[3], o1);
        } else {
#pragma unroll
          for (int j = 0; j < BA; ++j) {
            if constexpr (PERNB) {  // (the compiler's subtraction: no hand-written packed instruction)
              accum(acc[j * BP + s - 1], own0[j] - o0);
              accum(acc[j * BP + s - 1], own1[j] - o1);
            } else {
              accum(acc[j * BP + s - 1], vsub(own0[j], o0));
              accum(acc[j * BP + s - 1], vsub(own1[j], o1));
            }
          }
        }
      }
    }

    // ---- phase 3: covariances -> exchange matrix -> row per lane ---------------------------------------
    {
      T kv[NS];
      const T post_scale = post_scale_here();
      kernel_dispatch(a.kernel_id, a.metric_id, [&](auto kid, auto mid) {
        constexpr int KID = decltype(kid)::value, MID = decltype(mid)::value;
        if constexpr (sizeof(T) == 4) {
#pragma unroll
          for (int s = 0; s < NS; s += 2) {  // two covariances per packed instruction
            const f2 kk = cov_from_sqdist2(f2{acc_total(acc[s]), acc_total(acc[s + 1])}, KID, MID, post_scale);
            kv[s] = kk.x;
            kv[s + 1] = kk.y;
          }
        } else {
#pragma unroll
          for (int s = 0; s < NS; ++s) kv[s] = cov_from_sqdist<T>(acc_total(acc[s]), KID, MID, post_scale);
        }
      });
      const int dump = (NP - 1) * KS + NP;  // padding behind the last row
#pragma unroll
      for (int s = 1; s <= NS; ++s) {
        const int r1 = (i + own_offset((s - 1) / BP)) & (NP - 1);
        const int c = (i + (s - 1) % BP + 1) & (NP - 1);
        const int hi = max(r1, c), lo = min(r1, c);
        const bool real = lo < k && hi <= k;   // neighbour x neighbour, or neighbour x query
        Mh[hi <= k ? hi * KS + lo : dump] = real ? kv[s - 1] : T(0);
      }
      Mh[i * KS + i] = i < k ? T(1) + myeps : T(1);
    }
    __syncthreads();
    if (i < k) Mh[(k + 1) * KS + i] = myyt;      // the right-hand-side row (no pair store touches it)
    else if (i <= k + 1) Mh[(k + 1) * KS + i] = i == k + 1 ? T(1) : T(0);
    __syncthreads();
    V A[NP / E];
#pragma unroll
    for (int c4 = 0; c4 < NP / E; ++c4)
      A[c4] = i <= k + 1 ? *reinterpret_cast<const V*>(Mh + i * KS + c4 * E) : V(0);  // slots behind the rhs row: zero rows
    __syncthreads();

    // ---- phase 4: elimination, multipliers l_ij kept in the exchange matrix ---------------------------
    __builtin_amdgcn_s_setprio(2);  // chains of short dependent steps go first
    bool bad = false;
#pragma unroll
    for (int j = 0; j < (KFIX > 0 ? KFIX : NP - 2); ++j) {
      if (KFIX > 0 || j < k) {
        const T ajj = A[j / E][j % E];
        colh[i] = ajj;
        __syncthreads();
        const V cp = *reinterpret_cast<const V*>(colh + (j / E) * E);
        const T p = cp[j % E];
        bad = bad || !(p > T(0));
        const T t = ajj * pivot_rcp(p);
        Mh[i * KS + j] = t;
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
        __syncthreads();
      }
    }

    // ---- phase 5: back-substitution L^T [a w] = D^-1 L^-1 [c yt] ----------------------------------------
    T xa = i < k ? Mh[k * KS + i] : T(0);
    T xw = i < k ? Mh[(k + 1) * KS + i] : T(0);
    // Eight steps per block: the multipliers do not depend on the solution and are requested together, the updates
    // are selects, not branches -- a step that reads its multiplier inside a divergent `if` is a basic block of its
    // own with an LDS round trip in the open (29 of them per neighbourhood; the same cure as in mgp_fused_rhs.hip).
    {
      constexpr int BB = 8;
      constexpr int KTOP = KFIX > 0 ? KFIX : NP - 2;  // steps m = KTOP - 1 .. 1
#pragma unroll
      for (int mb = (KTOP - 1) / BB * BB; mb >= 0; mb -= BB) {
        if (KFIX > 0 || mb < k) {  // (uniform)
          T lm[BB];
#pragma unroll
          for (int e = 0; e < BB; ++e) lm[e] = Mh[(mb + e) * KS + i];
#pragma unroll
          for (int e = BB - 1; e >= 0; --e) {
            const int m = mb + e;
            if (m >= 1 && m < KTOP) {
              T am = lane_value(xa, m), wm = lane_value(xw, m);
              if constexpr (NH == 2) {
                const T am1 = lane_value(xa, m + NP), wm1 = lane_value(xw, m + NP);
                am = h == 0 ? am : am1;
                wm = h == 0 ? wm : wm1;
              }
              const bool on = i < m && (KFIX > 0 || m < k);
              xa = on ? fma_t(-lm[e], am, xa) : xa;
              xw = on ? fma_t(-lm[e], wm, xw) : xw;
            }
          }
        }
      }
    }
    __builtin_amdgcn_s_setprio(0);
    __syncthreads();  // every lane is done with the multipliers: M becomes the q matrix
    // (LOOCV: xw is u = K^-1 y so far; w = gm u from here on, u kept for the y^T K^-1 y terms)
    const T xu = xw;
    const T gyv = gyk ? gyk[nbb] : T(0);
    if (gyk) xw = (gmean ? gmean[nbb] : T(0)) * xu;
    T* uvec = colbuf;  // (free between the back-substitution and the next task's elimination)
    avec[lane] = i < k ? xa : T(0);
    wvec[lane] = i < k ? xw : T(0);
    if (gyk) uvec[lane] = i < k ? xu : T(0);
    __syncthreads();
    const bool skip = bad || !live || bad_scale;  // cotangents of a non-SPD neighbourhood are left untouched
    if constexpr (PERNB) {
      if (bad_scale && live) {  // (the whole half: its scale is one value)
        if (gnz && i < k) gnz[nb * k + i] = num<T>::nan();
        if (gls && i == 0) gls[nb] = num<T>::nan();
      }
    }

    // ---- phase 6: pair cotangents q_ij = gK_ij dkappa/dacc_ij, symmetric, zero diagonal ---------------
    const T gv = gvar ? gvar[nbb] : T(0);
    T liso = T(0);
    V s2h[HYPER ? DG : 1];  // (HYPER) per-feature sums of q_ij dz^2 over the lane's own pairs
    T qown[HYPER ? NS : 1];  // (HYPER) q of the lane's own pairs (zero for a pair that is not real, or met twice)
    {
      const T* ah = avec + h * NP;
      const T* wh = wvec + h * NP;
      const int dump = (NP - 1) * KS + NP;
      const T post_scale = post_scale_here();
      kernel_dispatch(a.kernel_id, a.metric_id, [&](auto kid, auto mid) {
        constexpr int KID = decltype(kid)::value, MID = decltype(mid)::value;
#pragma unroll
        for (int s = 1; s <= NS; ++s) {
          const int r1 = (i + own_offset((s - 1) / BP)) & (NP - 1);
          const int c = (i + (s - 1) % BP + 1) & (NP - 1);
          const int hi = max(r1, c), lo = min(r1, c);
          const bool real = lo < k && hi <= k;
          const T alo = ah[lo], wlo = wh[lo], ahi = ah[hi], whi = wh[hi];
          T gK = hi < k ? T(2) * gv * ahi * alo - (ahi * wlo + alo * whi) : wlo - T(2) * gv * alo;
          if (gyk && hi < k) gK -= T(2) * gyv * uvec[h * NP + hi] * uvec[h * NP + lo];
          const T accv = acc_total(acc[s - 1]);
          const T x = (MID == MGP_METRIC_L2 ? sqrt_fast(accv) : accv) * post_scale;
          // d kappa / d x with the fast exponential of the forward kernels (mgp_device.h: kernel_deriv)
          T kp;
          if constexpr (KID == MGP_KERNEL_RBF) kp = T(-0.5) * exp_neg(x * T(0.5));
          else if constexpr (KID == MGP_KERNEL_MATERN_05) kp = -exp_neg(x);
          else if constexpr (KID == MGP_KERNEL_MATERN_15) kp = T(-3) * x * exp_neg(x * T(1.7320508075688772935));
          else if constexpr (KID == MGP_KERNEL_MATERN_25) {
            const T t = x * T(2.2360679774997896964);
            kp = T(-5.0 / 3.0) * x * (T(1) + t) * exp_neg(t);
          } else kp = -x * exp_neg(x * x * T(0.5));
          T dk_dacc;
          if constexpr (MID == MGP_METRIC_L2) dk_dacc = x > T(0) ? kp * post_scale * post_scale * pivot_rcp(T(2) * x) : T(0);
          else dk_dacc = kp * post_scale;
          const T q = real ? gK * dk_dacc : T(0);
          // the pair at cyclic distance NP / 2 is met from both ends: count it once
          const bool twice = ((r1 - c) & (NP - 1)) == NP / 2 && r1 < c;
          if (real && !twice) liso += gK * kp * x;
          if constexpr (HYPER) {
            qown[s - 1] = (real && !twice) ? q : T(0);
          } else {
            Mh[hi <= k ? hi * KS + lo : dump] = q;
            Mh[hi <= k ? lo * KS + hi : dump] = q;
          }
        }
      });
      if constexpr (!HYPER) Mh[i * KS + i] = T(0);
    }
    if constexpr (HYPER) {
      // the pairs' shares of the per-feature length-scale partials, pair by pair (the distance accumulators are dead
      // by now; one copy of this loop, not one per covariance function)
#pragma unroll
      for (int c4 = 0; c4 < DG; ++c4) s2h[c4] = V(0);
      if (gls && aniso) {  // (uniform)
#pragma unroll
        for (int s = 1; s <= NS; ++s) {
          const int r1 = (i + own_offset((s - 1) / BP)) & (NP - 1);
          const int c = (i + (s - 1) % BP + 1) & (NP - 1);
          const V qv = V(qown[s - 1]);
          const T* xa_ = Xh + r1 * xs;
          const T* xb_ = Xh + c * xs;
#pragma unroll
          for (int c4 = 0; c4 < DG; ++c4) {
            const V dz = *reinterpret_cast<const V*>(xa_ + c4 * E) - *reinterpret_cast<const V*>(xb_ + c4 * E);
            s2h[c4] = (dz * qv) * dz + s2h[c4];
          }
          if ((s & 3) == 0) __builtin_amdgcn_sched_barrier(0);  // (four pairs' reads in flight; all hoisted, they spill)
        }
      }
    }
    // per-neighbourhood outputs that need a and w only
    if (!skip) {
      if (gnz && i < k) gnz[nb * k + i] = gv * xa * xa - xa * xw - gyv * xu * xu;
      if (gtg && gmean && i < k)
        for (int r = 0; r < R; ++r) unsafeAtomicAdd(gtg + myidx * (int64_t)R + r, gmean[nb * R + r] * xa + (gyk ? T(2) * gyv * xu : T(0)));
    }
    if (gls && !aniso) {
      // sum over the lanes of the half
      T s = liso;
      for (int off = NP / 2; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
      if (!skip && i == 0) gls[nb] = -(l2 ? T(1) : T(2)) * inv_l_here() * s;  // dx/dl = -x/l | -2x/l
    }
    __syncthreads();

    // ---- phase 7: feature cotangents: gx_i = 2 sum_j q_ij (x_i - x_j) (the metric's 1/l^2 is in q) ------
    const bool want_gl = gls && aniso;
    if constexpr (HYPER) {
      if (want_gl) {
        // every lane's pair sums through the tile, lane f adds column f (each unordered pair once: twice the sum)
        __syncthreads();
#pragma unroll
        for (int c4 = 0; c4 < DG; ++c4) *reinterpret_cast<V*>(Xh + i * xs + c4 * E) = s2h[c4];
        __syncthreads();
        for (int f = i; f < d; f += NP) {
          T acc = T(0);
          for (int j = 0; j < NP; ++j) acc += Xh[j * xs + f];
          if (!skip) gls[nb * (int64_t)d + f] = T(-2) * ilb[f] * acc;
        }
      }
    }
    if ((bad || bad_scale) && live && i == 0 && a.info) atomicAdd(a.info, 1);
  }
}

// the LDS carve, the grid and the residency rule of launch_bwd_np_impl
template <typename T, int NP, int DG>
static int launch_bwd_ns_np(const BackwardArgs& g, const void* ls_batch, hipStream_t stream) {
  constexpr int NH = 64 / NP;
  constexpr int E = v16<T>::N, KS = NP + E, xs = DG * E + E;
  const uintptr_t align = (uintptr_t)g.f.feat_q | (uintptr_t)g.f.feat_nn;
  const int vec_ok = (g.f.d % E == 0) && (align % 16 == 0);
  const size_t lds = ((size_t)NH * NP * xs + (size_t)NH * NP * KS + 4 * 64) * sizeof(T) + 64 * sizeof(int64_t);
  static Residency res;
  const LaunchLabel label(g.f.b, g.f.k, g.f.d, g.f.R, "mgp::ns_wave_backward_kernel<%s,%d,%d>", sizeof(T) == 4 ? "float" : "double", NP, DG);
  return launch_resident(&ns_wave_backward_kernel<T, NP, DG>, res, 64, lds, (g.f.b + NH - 1) / NH, nullptr, stream, &label, g, vec_ok,
                         NsLaunch{ls_batch}).status;
}

// by the row's 16-byte groups, as launch_bwd_dg (no compile-time nn_count: the headline shape's static form is the
// scalar launch's)
template <typename T, int NP>
int launch_bwd_ns_dg(const BackwardArgs& g, const void* ls_batch, hipStream_t stream) {
  constexpr int E = v16<T>::N;
  const int dv = (g.f.d + E - 1) / E;
  if (dv <= 4) return launch_bwd_ns_np<T, NP, 4>(g, ls_batch, stream);
  if (dv <= 8) return launch_bwd_ns_np<T, NP, 8>(g, ls_batch, stream);
  if constexpr (sizeof(T) == 8) {
    return MGP_EUNSUPPORTED;
  } else {
    if (dv <= 10) return launch_bwd_ns_np<T, NP, 10>(g, ls_batch, stream);
    if (dv <= 12) return launch_bwd_ns_np<T, NP, 12>(g, ls_batch, stream);
    return launch_bwd_ns_np<T, NP, 16>(g, ls_batch, stream);
  }
}

}  // namespace mgp
