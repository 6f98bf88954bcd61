// General-smoothness Matern, one covariance per lane, node count per lane GROUP (the prediction kernels of
// mgp_fast_mean.hip).  matern_gen_eval / matern_gen_batch64 (mgp_wave_common.h) run every lane to the longest tail of
// its WAVE: right where a wave is one neighbourhood, wrong where two test points share one -- a point's sum would
// pick up tail terms that depend on its partner.  Here a lane adds the terms below the node count of its own group of
// GW lanes (GW = 32: a half-wave; the cross-lane maximum stays inside the group) and nothing beyond, whatever the
// other group needs; the loop still ends on a wave ballot, so all 64 lanes make the call together.  A lane without
// a neighbour passes live = false: it is evaluated at x = 1 (no NaN can come out of it), counts no node towards its
// group and returns a value nobody reads.  Same node table, same launch constants (gen_launch_constants), same clamps
// and the same term arithmetic as the wave-wide evaluators; the masked sum restated in numpy float32:
// tests/test_fast_gen_cpu.py.
#pragma once
#include "mgp_wave_common.h"

namespace mgp {

// the largest value of the lane's group of GW consecutive lanes (GW a power of two up to 64)
template <int GW>
__device__ __forceinline__ int gen_group_max(int n) {
#pragma unroll
  for (int off = GW / 2; off > 0; off >>= 1) n = max(n, __shfl_xor(n, off, 64));
  return n;
}

// fp32: r = metric argument (scaled distance); lc = log2(h 2^(1-nu) / Gamma(nu)).  A zero distance returns exactly 1,
// a NaN distance stays NaN.
template <int GW>
__device__ __forceinline__ float matern_gen_eval_group(float r, bool live, const float* tab, float nu, float h, float lc) {
  const float s2nu = __builtin_amdgcn_sqrtf(2.0f * nu);
  float x = 1.0f;
  if (live) x = r != r ? r : __builtin_fminf(__builtin_fmaxf(r * s2nu, 1e-6f), 3.0e4f);
  const float lx = __builtin_amdgcn_logf(x);  // log2
  // nodes until x cosh t - nu t > ~22: T = ln(2 (22 + nu max(1, ln(44 / x))) / x)  (matern_gen_eval's rule)
  const float inner = 22.0f + nu * __builtin_fmaxf(1.0f, (5.4594316f - lx) * 0.693147181f);
  const float T = __builtin_fmaxf(1.0f, (__builtin_amdgcn_logf(2.0f * inner) - lx) * 0.693147181f);
  int N = (int)(T / h) + 3;  // (a NaN distance: fmax drops it, T = 1; its sum is NaN after the first node)
  N = N < MGP_GEN_NODES ? N : MGP_GEN_NODES;
  N = gen_group_max<GW>(live ? N : 0);
  const float L = __builtin_fmaf(nu, lx, lc);
  float acc = 0.0f;
  for (int n = 0; n < MGP_GEN_NODES; ++n) {
    if (__builtin_amdgcn_ballot_w64(n < N) == 0) break;  // (uniform: the longest tail of the wave's groups)
    const f2 cl = *reinterpret_cast<const f2*>(tab + 2 * n);  // uniform LDS read: (-c_n, l_n)
    const float e = __builtin_amdgcn_exp2f(__builtin_fmaf(x, cl.x, L + cl.y));
    acc += n < N ? e : 0.0f;  // (terms beyond the group's own count: not added)
  }
  return live && r == 0.0f ? 1.0f : acc;
}

// fp64: natural logarithms, the software exp of matern_gen_batch64, its zero-distance nudge and its clamps
template <int GW>
__device__ __forceinline__ double matern_gen_batch64_group(double v, bool live, const double* tab, double nu, double h, double lc,
                                                           double xmin) {
  constexpr auto C = [](unsigned long long bits) { return __builtin_bit_cast(double, bits); };
  const double s2nu = ::sqrt(2.0 * nu);
  double x = 1.0;
  if (live) {
    const double r = v == 0.0 ? 2.220446049250313e-16 : v;
    x = r != r ? r : __builtin_fmin(__builtin_fmax(r * s2nu, xmin), 1.0e5);
  }
  const double lx = ::log(x);
  const double tmax = __builtin_fmax(1.0, ::log(2.0 * (37.0 + nu * __builtin_fmax(1.0, 4.30406509320417 - lx))) - lx);
  int N = (int)(tmax / h) + 3;
  N = N < MGP_GEN_NODES64 ? N : MGP_GEN_NODES64;
  N = gen_group_max<GW>(live ? N : 0);
  const double L = __builtin_fma(nu, lx, lc);
  double acc = 0.0;
  for (int n = 0; n < MGP_GEN_NODES64; ++n) {
    if (__builtin_amdgcn_ballot_w64(n < N) == 0) break;  // (uniform: the longest tail of the wave's groups)
    const double negc = tab[2 * n], l = tab[2 * n + 1];  // uniform LDS reads
    const double t = -__builtin_fma(x, negc, L + l);
    const double m = __builtin_rint(t * -1.4426950408889634074);
    double r = __builtin_fma(m, -6.93147180369123816490e-01, -t);
    r = __builtin_fma(m, -1.90821492927058770002e-10, r);
    double q = fma_sc(r, C(0x3e5ae64567f544e4ull), C(0x3e928af3fca7ab0cull));
    constexpr unsigned long long coef[8] = {0x3ec71dee623fde64ull, 0x3efa01997c89e6b0ull, 0x3f2a01a014761f6eull, 0x3f56c16c1852b7b0ull,
                                            0x3f81111111122322ull, 0x3fa55555555502a1ull, 0x3fc5555555555511ull, 0x3fe000000000000bull};
#pragma unroll
    for (int c = 0; c < 8; ++c) q = fma_sc(q, r, C(coef[c]));
    q = __builtin_fma(q, r, 1.0);
    q = __builtin_fma(q, r, 1.0);
    const double e = __builtin_amdgcn_ldexp(q, cvt_i32_sat(m));
    acc += n < N ? e : 0.0;
  }
  return acc;
}

// ---- strips of pairs per lane, node count per lane group (the wave-sized backward, mgp_backward_wave_gen.h) -------------
// matern_gen_eval / matern_gen_batch64 / matern_gen_deriv_eval / matern_gen_deriv_batch64 with the node count of the
// lane's GROUP: the maximum over the live pairs of the group's lanes (gen_group_max; a group without a live pair counts
// none), the loop ends on a wave ballot, terms beyond the group's own count are not added (GW = 64: the count is the
// wave's and nothing is masked).  Tables, clamps, term arithmetic and zero-distance rules are those evaluators'.  The
// derivative forms take K0: the covariance itself (their s0 sum) as a third result, so that one pass serves a kernel
// that keeps k, dk/dr and dk/dnu; K0 or NU costs the second exponential per node, NU the third.

// nodes of one fp32 pair at log2 x = lx: x cosh t - w t > ~c0 (matern_gen_eval: c0 = 22, w = nu; the derivatives: 26, mu)
__device__ __forceinline__ float gen_span32(float lx, float w, float c0, float l2c) {
  const float inner = c0 + w * __builtin_fmaxf(1.0f, (l2c - lx) * 0.693147181f);
  return (__builtin_amdgcn_logf(2.0f * inner) - lx) * 0.693147181f;
}

__device__ __forceinline__ void f2_set(f2& v, int s, float a) {
  if (s & 1) v.y = a;
  else v.x = a;
}

template <int GW, int NS>
__device__ __forceinline__ void matern_gen_eval_strip_group(float (&r)[NS], unsigned live, const float* tab, float nu, float h, float lc) {
  static_assert(NS % 2 == 0, "pairs of covariances");
  f2 x2[NS / 2], L2[NS / 2], acc2[NS / 2];
  const float s2nu = __builtin_amdgcn_sqrtf(2.0f * nu);
  float nmaxf = 1.0f;
  unsigned zero = 0;
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const bool on = (live >> s) & 1u;
    float x = 1.0f;
    if (on) {
      if (r[s] == 0.0f) zero |= 1u << s;
      x = r[s] != r[s] ? r[s] : __builtin_fminf(__builtin_fmaxf(r[s] * s2nu, 1e-6f), 3.0e4f);
    }
    const float lx = __builtin_amdgcn_logf(x);
    if (on) nmaxf = __builtin_fmaxf(nmaxf, gen_span32(lx, nu, 22.0f, 5.4594316f));
    f2_set(x2[s / 2], s, x);
    f2_set(L2[s / 2], s, __builtin_fmaf(nu, lx, lc));
  }
  int N = (int)(nmaxf / h) + 3;
  N = N < MGP_GEN_NODES ? N : MGP_GEN_NODES;
  N = gen_group_max<GW>(live ? N : 0);
#pragma unroll
  for (int p = 0; p < NS / 2; ++p) acc2[p] = f2{0.0f, 0.0f};
  for (int n = 0; n < MGP_GEN_NODES; ++n) {
    if (__builtin_amdgcn_ballot_w64(n < N) == 0) break;  // (uniform: the longest tail of the wave's groups)
    const f2 cl = *reinterpret_cast<const f2*>(tab + 2 * n);
    const f2 negc = {cl.x, cl.x}, l = {cl.y, cl.y};
    const bool in = GW == 64 || n < N;
#pragma unroll
    for (int p = 0; p < NS / 2; ++p) {
      const f2 arg = x2[p] * negc + (L2[p] + l);
      f2 e;
      e.x = __builtin_amdgcn_exp2f(arg.x);
      e.y = __builtin_amdgcn_exp2f(arg.y);
      acc2[p] = acc2[p] + (in ? e : f2{0.0f, 0.0f});
    }
  }
#pragma unroll
  for (int s = 0; s < NS; ++s) r[s] = (zero >> s) & 1u ? 1.0f : (s & 1 ? acc2[s / 2].y : acc2[s / 2].x);
}

// in: r = metric arguments; out: r = dk/dr, K0: k0 = k (exactly 1 at zero distance), NU: dnu = dk/dnu
template <int GW, int NS, bool K0, bool NU>
__device__ __forceinline__ void matern_gen_deriv_strip_group(float (&r)[NS], float (&k0)[NS], float (&dnu)[NS], unsigned live,
                                                             const float* tab, const float* dtab, float nu, float h, float lc,
                                                             float psi) {
  static_assert(NS % 2 == 0, "pairs of covariances");
  f2 x2[NS / 2], L2[NS / 2], lx2[NS / 2], s1[NS / 2], s0[NS / 2], sd[NS / 2];
  const float s2nu = __builtin_amdgcn_sqrtf(2.0f * nu);
  const float mu = __builtin_fmaxf(nu, 1.0f - nu);
  float nmaxf = 1.0f;
  unsigned zero = 0;
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const bool on = (live >> s) & 1u;
    float x = 1.0f;
    if (on) {
      if (r[s] == 0.0f) zero |= 1u << s;
      x = r[s] != r[s] ? r[s] : __builtin_fminf(__builtin_fmaxf(r[s] * s2nu, 1e-6f), 3.0e4f);
    }
    const float lx = __builtin_amdgcn_logf(x);
    if (on) nmaxf = __builtin_fmaxf(nmaxf, gen_span32(lx, mu, 26.0f, 5.7004397f));
    f2_set(x2[s / 2], s, x);
    f2_set(L2[s / 2], s, __builtin_fmaf(nu, lx, lc));
    f2_set(lx2[s / 2], s, lx);
  }
  int N = (int)(nmaxf / h) + 3;
  N = N < MGP_GEN_NODES ? N : MGP_GEN_NODES;
  N = gen_group_max<GW>(live ? N : 0);
#pragma unroll
  for (int p = 0; p < NS / 2; ++p) s1[p] = s0[p] = sd[p] = f2{0.0f, 0.0f};
  for (int n = 0; n < MGP_GEN_NODES; ++n) {
    if (__builtin_amdgcn_ballot_w64(n < N) == 0) break;  // (uniform: the longest tail of the wave's groups)
    const f2 cl = *reinterpret_cast<const f2*>(tab + 2 * n);
    const f2 dl = *reinterpret_cast<const f2*>(dtab + 2 * n);
    const f2 negc = {cl.x, cl.x}, l1 = {dl.x, dl.x};
    const bool in = GW == 64 || n < N;
    const f2 none = {0.0f, 0.0f};
#pragma unroll
    for (int p = 0; p < NS / 2; ++p) {
      const f2 base = x2[p] * negc + L2[p];
      const f2 a1 = base + l1;
      f2 e;
      e.x = __builtin_amdgcn_exp2f(a1.x);
      e.y = __builtin_amdgcn_exp2f(a1.y);
      s1[p] = s1[p] + (in ? e : none);
      if constexpr (K0 || NU) {
        const f2 a0 = base + f2{cl.y, cl.y};
        e.x = __builtin_amdgcn_exp2f(a0.x);
        e.y = __builtin_amdgcn_exp2f(a0.y);
        s0[p] = s0[p] + (in ? e : none);
      }
      if constexpr (NU) {
        const f2 ad = base + f2{dl.y, dl.y};
        e.x = __builtin_amdgcn_exp2f(ad.x);
        e.y = __builtin_amdgcn_exp2f(ad.y);
        sd[p] = sd[p] + (in ? e : none);
      }
    }
  }
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const bool z = (zero >> s) & 1u;
    const float k1 = s & 1 ? s1[s / 2].y : s1[s / 2].x;
    const float kk = s & 1 ? s0[s / 2].y : s0[s / 2].x;
    r[s] = z ? 0.0f : -s2nu * k1;
    if constexpr (K0) k0[s] = z ? 1.0f : kk;
    if constexpr (NU) {
      const float kd = s & 1 ? sd[s / 2].y : sd[s / 2].x;
      const float x = s & 1 ? x2[s / 2].y : x2[s / 2].x, lx = s & 1 ? lx2[s / 2].y : lx2[s / 2].x;
      const float v = kk * (lx * 0.693147181f - 0.693147180559945f - psi) + kd - (x / (2.0f * nu)) * k1;
      dnu[s] = z ? 0.0f : v;
    }
  }
}

// fp64: the clamped scaled distance of one pair (the zero-distance nudge of matern_gen_batch64)
__device__ __forceinline__ double gen_scaled64(double v, bool on, double s2nu, double xmin) {
  if (!on) return 1.0;
  const double r = v == 0.0 ? 2.220446049250313e-16 : v;
  return r != r ? r : __builtin_fmin(__builtin_fmax(r * s2nu, xmin), 1.0e5);
}

template <int GW, int CB>
__device__ __forceinline__ void matern_gen_batch64_strip_group(double (&v)[CB], unsigned live, const double* tab, double nu, double h,
                                                               double lc, double xmin) {
  double x[CB], L[CB], acc[CB];
  const double s2nu = ::sqrt(2.0 * nu);
  double tmax = 1.0;
#pragma unroll
  for (int u = 0; u < CB; ++u) {
    const bool on = (live >> u) & 1u;
    x[u] = gen_scaled64(v[u], on, s2nu, xmin);
    const double lx = ::log(x[u]);
    if (on) tmax = __builtin_fmax(tmax, ::log(2.0 * (37.0 + nu * __builtin_fmax(1.0, 4.30406509320417 - lx))) - lx);
    L[u] = __builtin_fma(nu, lx, lc);
    acc[u] = 0.0;
  }
  int N = (int)(tmax / h) + 3;
  N = N < MGP_GEN_NODES64 ? N : MGP_GEN_NODES64;
  N = gen_group_max<GW>(live ? N : 0);
  for (int n = 0; n < MGP_GEN_NODES64; ++n) {
    if (__builtin_amdgcn_ballot_w64(n < N) == 0) break;  // (uniform: the longest tail of the wave's groups)
    const double negc = tab[2 * n], l = tab[2 * n + 1];
    const bool in = GW == 64 || n < N;
    double t[CB], e[CB];
#pragma unroll
    for (int u = 0; u < CB; ++u) t[u] = -__builtin_fma(x[u], negc, L[u] + l);
    gen_exp_neg_batch64<CB>(t, e);
#pragma unroll
    for (int u = 0; u < CB; ++u) acc[u] += in ? e[u] : 0.0;
  }
#pragma unroll
  for (int u = 0; u < CB; ++u) v[u] = acc[u];
}

template <int GW, int CB, bool K0, bool NU>
__device__ __forceinline__ void matern_gen_deriv_batch64_strip_group(double (&v)[CB], double (&k0)[CB], double (&dnu)[CB], unsigned live,
                                                                     const double* tab, const double* dtab, double nu, double h,
                                                                     double lc, double xmin, double psi) {
  double x[CB], L[CB], lxs[CB], s1[CB], s0[CB], sd[CB];
  const double s2nu = ::sqrt(2.0 * nu);
  const double mu = __builtin_fmax(nu, 1.0 - nu);
  double tmax = 1.0;
  unsigned zero = 0;
#pragma unroll
  for (int u = 0; u < CB; ++u) {
    const bool on = (live >> u) & 1u;
    if (on && v[u] == 0.0) zero |= 1u << u;
    x[u] = gen_scaled64(v[u], on, s2nu, xmin);
    const double lx = ::log(x[u]);
    if (on) tmax = __builtin_fmax(tmax, ::log(2.0 * (41.0 + mu * __builtin_fmax(1.0, 4.40671924726425 - lx))) - lx);
    lxs[u] = lx;
    L[u] = __builtin_fma(nu, lx, lc);
    s1[u] = s0[u] = sd[u] = 0.0;
  }
  int N = (int)(tmax / h) + 3;
  N = N < MGP_GEN_NODES64 ? N : MGP_GEN_NODES64;
  N = gen_group_max<GW>(live ? N : 0);
  for (int n = 0; n < MGP_GEN_NODES64; ++n) {
    if (__builtin_amdgcn_ballot_w64(n < N) == 0) break;  // (uniform: the longest tail of the wave's groups)
    const double negc = tab[2 * n], l1 = dtab[2 * n];
    const bool in = GW == 64 || n < N;
    double base[CB], t[CB], e[CB];
#pragma unroll
    for (int u = 0; u < CB; ++u) base[u] = __builtin_fma(x[u], negc, L[u]);
#pragma unroll
    for (int u = 0; u < CB; ++u) t[u] = -(base[u] + l1);
    gen_exp_neg_batch64<CB>(t, e);
#pragma unroll
    for (int u = 0; u < CB; ++u) s1[u] += in ? e[u] : 0.0;
    if constexpr (K0 || NU) {
      const double l0 = tab[2 * n + 1];
#pragma unroll
      for (int u = 0; u < CB; ++u) t[u] = -(base[u] + l0);
      gen_exp_neg_batch64<CB>(t, e);
#pragma unroll
      for (int u = 0; u < CB; ++u) s0[u] += in ? e[u] : 0.0;
    }
    if constexpr (NU) {
      const double ld = dtab[2 * n + 1];
#pragma unroll
      for (int u = 0; u < CB; ++u) t[u] = -(base[u] + ld);
      gen_exp_neg_batch64<CB>(t, e);
#pragma unroll
      for (int u = 0; u < CB; ++u) sd[u] += in ? e[u] : 0.0;
    }
  }
#pragma unroll
  for (int u = 0; u < CB; ++u) {
    const bool z = (zero >> u) & 1u;
    v[u] = z ? 0.0 : -s2nu * s1[u];
    if constexpr (K0) k0[u] = s0[u];  // (a zero distance is the reference's eps, as in matern_gen_batch64)
    if constexpr (NU) {
      const double w = s0[u] * (lxs[u] - 0.693147180559945309417 - psi) + sd[u] - (x[u] / (2.0 * nu)) * s1[u];
      dnu[u] = z ? 0.0 : w;
    }
  }
}

}  // namespace mgp
