// Hyper-parameter backward of the general-smoothness Matern at wave size (mgp_hyper_backward_gen_wave_*): k + 2 <= 64
// slots, the partials d loss / d l (scalar or per feature), d loss / d eps and d loss / d nu alone.
//
// A kernel of its own, in translation units of its own (mgp_backward_wave_gen.hip, mgp_backward_wave_gen_f32.hip), on
// the phases and the LDS carve of ns_wave_backward_kernel (mgp_backward_wave_ns.h; mgp_backward_wave_kernel.h states the
// maths): gather -> cyclic register-blocked pair distances -> covariances -> exchange -> row-per-lane elimination ->
// back-substitution -> pair cotangents.  It is not an instantiation of that kernel's text, nor of backward_wave_kernel's
// or fused_wave_kernel's: those bodies sit within a few registers of their caps and sharing text moves every existing
// instantiation's allocation.
//
// What is this kernel's own:
//   - the covariance function and its derivatives come from the quadrature evaluators, in strips of
//     gen_pairs_per_call<T>() of the lane's NS = NP / 2 pairs (a compile-time count: every lane makes the same number
//     of calls), with the node count of the lane's HALF when two neighbourhoods share the wave (mgp_gen_group.h): a
//     neighbourhood's bits do not depend on its partner.  Slots that are no real pair, and the dead half of an odd
//     tail, are evaluated at x = 1 and drive no node count.
//   - recompute or keep (KEEP below).  fp32 keeps: ONE pass of the derivative evaluator in phase 3 yields k (its s0
//     sum), dk/dr and dk/dnu; what phase 6 needs of a pair -- kp x under Isotropy, dk/dacc under Anisotropy, and dk/dnu
//     -- is two registers, as many as the pair's distance accumulator that dies in their place.  fp64 recomputes: the
//     row of the system is 64 / 128 registers already, the distances stay and the derivative pass runs in phase 6
//     behind the back-substitution, the forward evaluator in phase 3 (the forward kernels' own bits at a zero distance).
//   - grad_nu: lnu += gK dk/dnu per pair, closed with the in-half butterfly of the isotropic sum (fixed order, no
//     floating-point atomic).  A pair at zero distance gets 0 for both derivatives from the evaluators.
//   - both node tables sit behind the carve, built once per workgroup; the derivative table only where it is read.
#pragma once
#include "mgp_assemble.h"
#include "mgp_gen_group.h"
#include "mgp_gen_launch.h"
#include "mgp_launch.h"
#include "mgp_wave_common.h"

namespace mgp {

// which form an instantiation takes (DESIGN sec. 4.5 has the resource records behind it)
template <typename T, int NP>
constexpr bool gen_wave_backward_keeps() { return sizeof(T) == 4; }

// One strip of a lane's pairs through the evaluators, node count per group of GW lanes.  In: v = metric arguments.
// FWD: v = k alone.  Otherwise v = dk/dr, k0 = k (K0), dn = dk/dnu (NU).
template <typename T, int GW, bool FWD, bool K0, bool NU>
__device__ __forceinline__ void gen_wave_strip(T (&v)[gen_pairs_per_call<T>()], T (&k0)[gen_pairs_per_call<T>()],
                                               T (&dn)[gen_pairs_per_call<T>()], unsigned live, double nu, const GenLaunch& g,
                                               const T* tab, const T* dtab) {
  constexpr int PC = gen_pairs_per_call<T>();
  if constexpr (sizeof(T) == 4) {
    if constexpr (FWD) matern_gen_eval_strip_group<GW, PC>(v, live, tab, (float)nu, g.h, g.lc);
    else matern_gen_deriv_strip_group<GW, PC, K0, NU>(v, k0, dn, live, tab, dtab, (float)nu, g.h, g.lc, (float)g.psi);
  } else {
    if constexpr (FWD) matern_gen_batch64_strip_group<GW, PC>(v, live, tab, nu, g.h64, g.lc64, g.xmin64);
    else matern_gen_deriv_batch64_strip_group<GW, PC, K0, NU>(v, k0, dn, live, tab, dtab, nu, g.h64, g.lc64, g.xmin64, g.psi);
  }
}

// Waves per SIMD the register allocation is held to: what the LDS of a workgroup admits anyway (160 KiB per CU, four
// SIMDs) -- two where tile, exchange matrix and tables stay below 20 KiB (fp32 at 32 slots and up to 16 features), one
// elsewhere, which leaves the allocator the whole register file.
template <typename T, int NP, int DG>
constexpr int gen_wave_backward_waves() { return sizeof(T) == 4 && NP == 32 && DG <= 4 ? 2 : 1; }

// DG: 16-byte groups of a (zero-padded) feature row; NU: grad_nu is written
template <typename T, int NP, int DG, bool NU>
__global__ __launch_bounds__(64, (gen_wave_backward_waves<T, NP, DG>())) void gen_wave_backward_kernel(BackwardArgs g, T* gnu, int vec_ok,
                                                                                                     GenLaunch gl) {
  constexpr bool KEEP = gen_wave_backward_keeps<T, NP>();
  constexpr int PC = gen_pairs_per_call<T>();
  constexpr int NH = 64 / NP;
  constexpr int NS = NP / 2, BA = 4, BP = NS / BA;
  static_assert(NS % PC == 0, "whole strips");
  auto own_offset = [](int j) { return j == 0 ? 0 : (j + 1) * BP + 1; };
  constexpr int E = v16<T>::N, CH = 2 * E, KS = NP + E;
  constexpr int xs = DG * E + E;  // odd number of 16-byte slots per tile row
  using V = typename v16<T>::type;
  using ACC = typename v16<T>::acc;
  const FusedArgs& a = g.f;
  const int k = a.k, d = a.d, R = a.R;

  extern __shared__ __attribute__((aligned(16))) char smem[];
  T* X = reinterpret_cast<T*>(smem);             // NH * NP rows x xs
  T* M = X + NH * NP * xs;                       // NH x NP x KS: exchange matrix, then the multipliers
  T* colbuf = M + NH * NP * KS;                  // 64
  T* avec = colbuf + 64;                         // 64
  T* wvec = avec + 64;                           // 64
  T* ilb = wvec + 64;                            // 64: inverse length scales (Anisotropy; zero past d)
  int64_t* idxbuf = reinterpret_cast<int64_t*>(ilb + 64);  // 64 row offsets (elements)
  const T* tab = reinterpret_cast<const T*>(smem + gl.tab);    // node table of the forward, behind the carve
  const T* dtab = reinterpret_cast<const T*>(smem + gl.dtab);  // ... and of the derivatives

  const T* feat_q = static_cast<const T*>(a.feat_q);
  const T* feat_nn = static_cast<const T*>(a.feat_nn);
  const T* targets = static_cast<const T*>(a.targets);
  const T* noise_dev = static_cast<const T*>(a.noise_dev);
  const T* gmean = static_cast<const T*>(g.grad_mean);
  const T* gvar = static_cast<const T*>(g.grad_var);
  const T* gyk = static_cast<const T*>(g.grad_yk);  // (LOOCV, R = 1: the right-hand side is y, w = gm u below)
  T* gls = static_cast<T*>(g.grad_ls);
  T* gnz = static_cast<T*>(g.grad_noise);
  const bool l2 = a.metric_id == MGP_METRIC_L2;
  const bool aniso = a.ls_count > 1;
  const bool want_d = gls || NU;  // (uniform) the derivatives are read
  const T inv_l = aniso ? T(1) : T(1) / static_cast<const T*>(a.length_scale)[0];
  const T post_scale = l2 ? inv_l : inv_l * inv_l;
  if (aniso) {
    const int f = threadIdx.x;
    ilb[f] = f < a.d ? T(1) / static_cast<const T*>(a.length_scale)[f] : T(0);
  }
  // (both tables are visible behind the task loop's first barrier)
  gen_build_node_table<T>(reinterpret_cast<T*>(smem + gl.tab), a.smoothness, gl, (int)threadIdx.x);
  if (KEEP || want_d) gen_build_deriv_node_table<T>(reinterpret_cast<T*>(smem + gl.dtab), a.smoothness, gl, (int)threadIdx.x);
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
    int64_t myidx = 0;
    T myeps = T(0), myyt = T(0);
    if (i < k) {
      myidx = a.nn_idx[nbb * k + i];
      if (a.noise_mode == MGP_NOISE_SCALAR) myeps = (T)a.noise_scalar;
      else if (a.noise_mode == MGP_NOISE_TABLE) myeps = noise_dev[myidx];
      else myeps = noise_dev[nbb * k + i];
      if (gyk) {
        myyt = targets[myidx * (int64_t)R];
      } else if (gmean) {
        const T* ty = targets + myidx * (int64_t)R;
        for (int r = 0; r < R; ++r) myyt += gmean[nbb * R + r] * ty[r];
      }
    } else if (i == k) {
      myidx = a.batch_idx ? a.batch_idx[nbb] : nbb;
    }
    __syncthreads();
    idxbuf[lane] = myidx * (int64_t)d;
    __syncthreads();

    // ---- phase 1: feature tile (rows 0 .. k of each half; other slots zero rows) ---------------------
    for (int t = lane; t < NH * NP * DG; t += 64) {
      const int row = t / DG, c = t - row * DG;
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
    __syncthreads();
    if (aniso) {  // z = x / l, in place
      T* xrow = Xh + i * xs;
#pragma unroll
      for (int c4 = 0; c4 < DG; ++c4) {
        V x = *reinterpret_cast<const V*>(xrow + c4 * E);
        x = x * *reinterpret_cast<const V*>(ilb + c4 * E);
        *reinterpret_cast<V*>(xrow + c4 * E) = x;
      }
      __syncthreads();
    }

    // ---- phase 2: squared distances of the lane's NS pairs ------------------------------------------
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
        if constexpr (sizeof(T) == 4) {
          // hand-ordered packed blocks: no instruction reads its predecessor's result (mgp_wave_common.h)
          dist_block4(acc[s - 1], acc[BP + s - 1], acc[2 * BP + s - 1], acc[3 * BP + s - 1], own0[0], own0[1], own0[2], own0[3], o0);
          dist_block4(acc[s - 1], acc[BP + s - 1], acc[2 * BP + s - 1], acc[3 * BP + s - 1], own1[0], own1[1], own1[2], own1[3], o1);
        } else {
#pragma unroll
          for (int j = 0; j < BA; ++j) {
            accum(acc[j * BP + s - 1], own0[j] - o0);
            accum(acc[j * BP + s - 1], own1[j] - o1);
          }
        }
      }
    }

    __builtin_amdgcn_sched_barrier(0);  // (nothing of the covariance phase moves up between the distance blocks)

    // the pair in the lane's slot s (0-based): its rows, whether it is a pair of the system, whether it is the copy of
    // a pair met from both ends (cyclic distance NP / 2: counted once)
    auto pair_of = [&](int s, int& hi, int& lo, bool& real, bool& twice) {
      const int r1 = (i + own_offset(s / BP)) & (NP - 1);
      const int c = (i + s % BP + 1) & (NP - 1);
      hi = max(r1, c), lo = min(r1, c);
      real = lo < k && hi <= k;  // neighbour x neighbour, or neighbour x query
      twice = ((r1 - c) & (NP - 1)) == NP / 2 && r1 < c;
    };
    // the metric arguments of one strip and its live mask
    auto strip_args = [&](int s0, T (&v)[PC]) -> unsigned {
      unsigned lv = 0;
#pragma unroll
      for (int u = 0; u < PC; ++u) {
        int hi, lo;
        bool real, twice;
        pair_of(s0 + u, hi, lo, real, twice);
        v[u] = acc_total(acc[s0 + u]);
        if (real && live) lv |= 1u << u;
      }
      if constexpr (sizeof(T) == 4) {
#pragma unroll
        for (int u = 0; u < PC; ++u) v[u] = (l2 ? sqrt_fast(v[u]) : v[u]) * post_scale;
      } else {
        if (l2) metric_batch64<PC, MGP_METRIC_L2>(v, post_scale);
        else metric_batch64<PC, MGP_METRIC_F2>(v, post_scale);
      }
      return lv;
    };
    // what phase 6 reads of a pair: kp x (Isotropy: its share of the scalar partial) or dk/dacc (Anisotropy)
    auto ls_term = [&](T x, T kp) -> T {
      if (!aniso) return kp * x;
      if (l2) return x > T(0) ? kp * post_scale * post_scale * pivot_rcp(T(2) * x) : T(0);
      return kp * post_scale;
    };

    // ---- phase 3: covariances -> exchange matrix -> row per lane ---------------------------------------
    T dls[KEEP ? NS : 1], dnk[KEEP && NU ? NS : 1];  // (KEEP) ls_term and dk/dnu of the lane's pairs
    {
      const int dump = (NP - 1) * KS + NP;  // padding behind the last row
#pragma unroll
      for (int s0 = 0; s0 < NS; s0 += PC) {
        T v[PC], k0[PC], dn[PC];
        const unsigned lv = strip_args(s0, v);
        if constexpr (KEEP) {
          T x[PC];
#pragma unroll
          for (int u = 0; u < PC; ++u) x[u] = v[u];
          gen_wave_strip<T, NP, false, true, NU>(v, k0, dn, lv, a.smoothness, gl, tab, dtab);
#pragma unroll
          for (int u = 0; u < PC; ++u) {
            dls[s0 + u] = ls_term(x[u], v[u]);
            if constexpr (NU) dnk[s0 + u] = dn[u];
          }
        } else {
          gen_wave_strip<T, NP, true, false, false>(v, k0, dn, lv, a.smoothness, gl, tab, dtab);
#pragma unroll
          for (int u = 0; u < PC; ++u) k0[u] = v[u];
        }
#pragma unroll
        for (int u = 0; u < PC; ++u) {
          int hi, lo;
          bool real, twice;
          pair_of(s0 + u, hi, lo, real, twice);
          Mh[hi <= k ? hi * KS + lo : dump] = real ? k0[u] : T(0);
        }
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
    for (int j = 0; j < NP - 2; ++j) {
      if (j < k) {
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

    // ---- phase 5: back-substitution L^T [a w] = D^-1 L^-1 [c yt], eight steps per block ----------------
    T xa = i < k ? Mh[k * KS + i] : T(0);
    T xw = i < k ? Mh[(k + 1) * KS + i] : T(0);
    {
      constexpr int BB = 8;
      constexpr int KTOP = NP - 2;  // steps m = KTOP - 1 .. 1
#pragma unroll
      for (int mb = (KTOP - 1) / BB * BB; mb >= 0; mb -= BB) {
        if (mb < k) {  // (uniform)
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
              const bool on = i < m && m < k;
              xa = on ? fma_t(-lm[e], am, xa) : xa;
              xw = on ? fma_t(-lm[e], wm, xw) : xw;
            }
          }
        }
      }
    }
    __builtin_amdgcn_s_setprio(0);
    __syncthreads();
    // (LOOCV: xw is u = K^-1 y so far; w = gm u from here on, u kept for the y^T K^-1 y terms)
    const T xu = xw;
    const T gyv = gyk ? gyk[nbb] : T(0);
    if (gyk) xw = (gmean ? gmean[nbb] : T(0)) * xu;
    T* uvec = colbuf;  // (free between the back-substitution and the next task's elimination)
    avec[lane] = i < k ? xa : T(0);
    wvec[lane] = i < k ? xw : T(0);
    if (gyk) uvec[lane] = i < k ? xu : T(0);
    __syncthreads();
    const bool skip = bad || !live;  // the rows of a non-SPD neighbourhood are left untouched

    // ---- phase 6: per pair q = gK x (its length-scale term), lnu += gK dk/dnu --------------------------
    __builtin_amdgcn_sched_barrier(0);
    const T gv = gvar ? gvar[nbb] : T(0);
    T lsum = T(0), lnu = T(0);
    T qown[NS];  // q of the lane's own pairs (zero for a pair that is not real, or met twice)
    if (KEEP || want_d) {  // (uniform)
      const T* ah = avec + h * NP;
      const T* wh = wvec + h * NP;
#pragma unroll
      for (int s0 = 0; s0 < NS; s0 += PC) {
        T dl[PC], dn[PC];
        if constexpr (KEEP) {
#pragma unroll
          for (int u = 0; u < PC; ++u) {
            dl[u] = dls[s0 + u];
            dn[u] = NU ? dnk[NU ? s0 + u : 0] : T(0);
          }
        } else {
          T v[PC], x[PC], k0[PC];
          const unsigned lv = strip_args(s0, v);
#pragma unroll
          for (int u = 0; u < PC; ++u) x[u] = v[u], dn[u] = T(0);
          gen_wave_strip<T, NP, false, false, NU>(v, k0, dn, lv, a.smoothness, gl, tab, dtab);
#pragma unroll
          for (int u = 0; u < PC; ++u) dl[u] = ls_term(x[u], v[u]);
        }
#pragma unroll
        for (int u = 0; u < PC; ++u) {
          int hi, lo;
          bool real, twice;
          pair_of(s0 + u, hi, lo, real, twice);
          const T alo = ah[lo], wlo = wh[lo], ahi = ah[hi], whi = wh[hi];
          T gK = hi < k ? T(2) * gv * ahi * alo - (ahi * wlo + alo * whi) : wlo - T(2) * gv * alo;
          if (gyk && hi < k) gK -= T(2) * gyv * uvec[h * NP + hi] * uvec[h * NP + lo];
          const bool once = real && !twice;
          const T q = once ? gK * dl[u] : T(0);
          qown[s0 + u] = q;
          lsum += q;
          if constexpr (NU) lnu += once ? gK * dn[u] : T(0);
        }
      }
    }
    // the pairs' shares of the per-feature length-scale partials, pair by pair (the distance accumulators are dead)
    V s2h[DG];
#pragma unroll
    for (int c4 = 0; c4 < DG; ++c4) s2h[c4] = V(0);
    if (gls && aniso) {  // (uniform)
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        const int r1 = (i + own_offset(s / BP)) & (NP - 1);
        const int c = (i + s % BP + 1) & (NP - 1);
        const V qv = V(qown[s]);
        const T* xa_ = Xh + r1 * xs;
        const T* xb_ = Xh + c * xs;
#pragma unroll
        for (int c4 = 0; c4 < DG; ++c4) {
          const V dz = *reinterpret_cast<const V*>(xa_ + c4 * E) - *reinterpret_cast<const V*>(xb_ + c4 * E);
          s2h[c4] = (dz * qv) * dz + s2h[c4];
        }
        if ((s & 3) == 3) __builtin_amdgcn_sched_barrier(0);  // (four pairs' reads in flight; all hoisted, they spill)
      }
    }
    if (!skip && gnz && i < k) gnz[nb * k + i] = gv * xa * xa - xa * xw - gyv * xu * xu;
    if (gls && !aniso) {  // the sum over the lanes of the half, a fixed order
      T s = lsum;
      for (int off = NP / 2; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
      if (!skip && i == 0) gls[nb] = -(l2 ? T(1) : T(2)) * inv_l * s;  // dx/dl = -x/l | -2x/l
    }
    if constexpr (NU) {
      T s = lnu;
      for (int off = NP / 2; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
      if (gnu && !skip && i == 0) gnu[nb] = s;
    }
    __syncthreads();

    // ---- phase 7: per-feature partials: every lane's pair sums through the tile, lane f adds column f ----
    if (gls && aniso) {
#pragma unroll
      for (int c4 = 0; c4 < DG; ++c4) *reinterpret_cast<V*>(Xh + i * xs + c4 * E) = s2h[c4];
      __syncthreads();
      for (int f = i; f < d; f += NP) {
        T sum = T(0);
        for (int j = 0; j < NP; ++j) sum += Xh[j * xs + f];
        if (!skip) gls[nb * (int64_t)d + f] = T(-2) * ilb[f] * sum;
      }
    }
    if (bad && live && i == 0 && a.info) atomicAdd(a.info, 1);
  }
}

// the LDS carve of launch_bwd_ns_np with both node tables behind it, its grid and its residency rule
template <typename T, int NP, int DG, bool NU>
static int launch_bwd_gen_np(const BackwardArgs& g, T* gnu, hipStream_t stream) {
  constexpr int NH = 64 / NP;
  constexpr int E = v16<T>::N, KS = NP + E, xs = DG * E + E;
  const uintptr_t align = (uintptr_t)g.f.feat_q | (uintptr_t)g.f.feat_nn;
  const int vec_ok = (g.f.d % E == 0) && (align % 16 == 0);
  const size_t carve = ((size_t)NH * NP * xs + (size_t)NH * NP * KS + 4 * 64) * sizeof(T) + 64 * sizeof(int64_t);
  GenLaunch gl = gen_launch_constants(g.f.smoothness, sizeof(T) == 8);
  gl.tab = (int)carve;
  gl.dtab = gl.tab + (int)gen_table_bytes(sizeof(T));
  const size_t lds = carve + gen_table_bytes(sizeof(T)) + gen_deriv_table_bytes(sizeof(T));
  static Residency res;
  const LaunchLabel label(g.f.b, g.f.k, g.f.d, g.f.R, "mgp::gen_wave_backward_kernel<%s,%d,%d,%s>", sizeof(T) == 4 ? "float" : "double", NP,
                          DG, NU ? "true" : "false");
  return launch_resident(&gen_wave_backward_kernel<T, NP, DG, NU>, res, 64, lds, (g.f.b + NH - 1) / NH, nullptr, stream, &label, g, gnu,
                         vec_ok, gl).status;
}

// Which of the two forms (grad_nu written or not) an (element size, slot count, row width) is served by: only
// instantiations whose resource record shows no spilled register and no scratch are built.
//   fp64, 64 slots, with grad_nu: spills (the row alone is 128 registers)            -> MGP_EUNSUPPORTED
//   fp32, 64 slots, more than 40 features, with grad_nu: spills                      -> MGP_EUNSUPPORTED
//   fp64, 32 slots, without grad_nu: that form spills four registers, the other none -> the NU form, gnu = NULL
template <typename T, int NP, int DG>
static int launch_bwd_gen_nu(const BackwardArgs& g, void* grad_nu, hipStream_t stream) {
  if constexpr ((sizeof(T) == 8 && NP == 64) || (sizeof(T) == 4 && NP == 64 && DG > 10)) {
    if (grad_nu) return MGP_EUNSUPPORTED;
    return launch_bwd_gen_np<T, NP, DG, false>(g, static_cast<T*>(nullptr), stream);
  } else if constexpr (sizeof(T) == 8) {
    return launch_bwd_gen_np<T, NP, DG, true>(g, static_cast<T*>(grad_nu), stream);
  } else {
    if (grad_nu) return launch_bwd_gen_np<T, NP, DG, true>(g, static_cast<T*>(grad_nu), stream);
    return launch_bwd_gen_np<T, NP, DG, false>(g, static_cast<T*>(nullptr), stream);
  }
}

// by the row's 16-byte groups, as launch_bwd_ns_dg
template <typename T, int NP>
int launch_bwd_gen_dg(const BackwardArgs& g, void* grad_nu, hipStream_t stream) {
  constexpr int E = v16<T>::N;
  const int dv = (g.f.d + E - 1) / E;
  if (dv <= 4) return launch_bwd_gen_nu<T, NP, 4>(g, grad_nu, stream);
  if constexpr (sizeof(T) == 8) {
    if constexpr (NP == 32) {
      if (dv <= 8) return launch_bwd_gen_nu<T, NP, 8>(g, grad_nu, stream);
    }
    return MGP_EUNSUPPORTED;
  } else {
    if (dv <= 8) return launch_bwd_gen_nu<T, NP, 8>(g, grad_nu, stream);
    if (dv <= 10) return launch_bwd_gen_nu<T, NP, 10>(g, grad_nu, stream);
    if (dv <= 12) return launch_bwd_gen_nu<T, NP, 12>(g, grad_nu, stream);
    return launch_bwd_gen_nu<T, NP, 16>(g, grad_nu, stream);
  }
}

}  // namespace mgp
