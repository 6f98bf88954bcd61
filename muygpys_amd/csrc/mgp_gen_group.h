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

}  // namespace mgp
