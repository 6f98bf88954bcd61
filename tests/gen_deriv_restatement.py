"""numpy restatements of the derivative evaluators of the general-smoothness Matern (csrc/mgp_wave_common.h:
``matern_gen_deriv_eval`` / ``gen_build_deriv_table`` in fp32, ``matern_gen_deriv_batch64`` / ``gen_build_deriv_table64``
in fp64), statement for statement at the working precision, and their scipy references.  Shared by
tests/test_matern_gen_deriv_cpu.py and the fp64 reference of tests/test_gpu_gen_backward.py.

With x = sqrt(2 nu) r, c = 2^(1-nu) / Gamma(nu), k = c x^nu K_nu(x):

    dk/dr      = -sqrt(2 nu) c x^nu K_{nu-1}(x)
    dk/dnu |_r = k (ln x - ln 2 - psi(nu)) + c x^nu dK_nu/dnu + (x / (2 nu)) dk/dx,   dk/dx = -c x^nu K_{nu-1}(x)
    dK_nu/dnu  = int_0^inf exp(-x cosh t) t sinh(nu t) dt

Every pair gets its OWN node count here (on the device a pair runs to the largest count of its wave, which is never
fewer nodes): the worst case of the truncated rule."""

import math

import numpy as np

LN2 = 0.693147180559945309417
LOG2E = 1.44269504088896
NO_TERM = -1.0e4  # the logarithm of a node weight that is zero (node 0 of t sinh(nu t))


def gen_step(nu):
    return 0.5 if nu <= 2.0 else (0.4 if nu <= 4.0 else (0.3 if nu <= 10.0 else 0.22))


def gen_step64(nu):
    return 0.30 if nu <= 2.0 else (0.25 if nu <= 4.0 else (0.18 if nu <= 10.0 else 0.13))


def gen_span64(x, nu):
    lx = np.log(x)
    return np.log(2.0 * (37.0 + nu * np.maximum(1.0, 4.30406509320417 - lx))) - lx


def gen_xmin64(nu, nodes=256):
    reach = (nodes - 4) * gen_step64(nu)
    lo, hi = -300.0, 0.0
    for _ in range(80):
        mid = 0.5 * (lo + hi)
        if gen_span64(10.0**mid, nu) > reach:
            lo = mid
        else:
            hi = mid
    return 10.0**hi


def digamma_host(x):
    """gen_digamma of csrc/mgp_gen_launch.h: the recurrence up to x >= 10, then the asymptotic series."""
    s = 0.0
    while x < 10.0:
        s -= 1.0 / x
        x += 1.0
    f = 1.0 / (x * x)
    return s + math.log(x) - 0.5 / x - f * (1.0 / 12 - f * (1.0 / 120 - f * (1.0 / 252 - f * (1.0 / 240 - f * (1.0 / 132)))))


def deriv_fp32(r, nu, want_nu=True, truncate=True):
    """(dk/dr, dk/dnu or None) in numpy float32.  ``truncate=False``: the whole 128-node table."""
    f = np.float32
    h = f(gen_step(nu))
    nuf = f(nu)
    t = np.arange(128, dtype=f) * h
    a = nuf * t
    negc = (-np.cosh(t) * f(LOG2E)).astype(f)
    l = ((a + np.log1p(np.exp(f(-2.0) * a)) - f(LN2)) * f(LOG2E)).astype(f)
    l[0] -= f(1.0)
    b = np.abs(nuf - f(1.0)) * t
    l1 = ((b + np.log1p(np.exp(f(-2.0) * b)) - f(LN2)) * f(LOG2E)).astype(f)
    l1[0] -= f(1.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        ls = ((np.log(t) + a + np.log(-np.expm1(f(-2.0) * a)) - f(LN2)) * f(LOG2E)).astype(f)
    ls[0] = f(NO_TERM)
    lc = f((np.log(float(h)) + (1.0 - nu) * np.log(2.0) - math.lgamma(nu)) / np.log(2.0))
    psi = f(digamma_host(nu))
    r = np.asarray(r, dtype=f)
    s2nu = np.sqrt(f(2.0) * nuf)
    x = np.minimum(np.maximum(r * s2nu, f(1e-6)), f(3.0e4)).astype(f)
    lx = np.log2(x).astype(f)
    mu = np.maximum(nuf, f(1.0) - nuf)  # the slowest-decaying weight: cosh((1 - nu) t) below nu = 1/2
    inner = f(26.0) + mu * np.maximum(f(1.0), (f(5.7004397) - lx) * f(0.693147181))
    T = (np.log2(f(2.0) * inner).astype(f) - lx) * f(0.693147181)
    N = np.minimum((np.maximum(T, f(1.0)) / h).astype(np.int64) + 3, 128)
    if not truncate:
        N = np.full_like(N, 128)
    L = (nuf * lx + lc).astype(f)
    s1 = np.zeros_like(x)
    s0 = np.zeros_like(x)
    sd = np.zeros_like(x)
    for i in range(int(N.max())):
        on = i < N
        base = (x * negc[i] + L).astype(f)
        s1 = s1 + np.where(on, np.exp2((base + l1[i]).astype(f)), f(0)).astype(f)
        if want_nu:
            s0 = s0 + np.where(on, np.exp2((base + l[i]).astype(f)), f(0)).astype(f)
            sd = sd + np.where(on, np.exp2((base + ls[i]).astype(f)), f(0)).astype(f)
    zero = r == 0
    dr = np.where(zero, f(0), -s2nu * s1).astype(f)
    if not want_nu:
        return dr, None
    dnu = (s0 * (lx * f(0.693147181) - f(LN2) - psi) + sd - (x / (f(2.0) * nuf)) * s1).astype(f)
    return dr, np.where(zero, f(0), dnu).astype(f)


def deriv_fp64(r, nu, want_nu=True, truncate=True, nodes=256):
    """(dk/dr, dk/dnu or None) in numpy float64 (np.exp standing in for the kernel's software exp)."""
    h = gen_step64(nu)
    t = np.arange(nodes) * h
    a = nu * t
    negc = -np.cosh(t)
    l = a + np.log1p(np.exp(-2.0 * a)) - LN2
    l[0] -= LN2
    b = abs(nu - 1.0) * t
    l1 = b + np.log1p(np.exp(-2.0 * b)) - LN2
    l1[0] -= LN2
    with np.errstate(divide="ignore", invalid="ignore"):
        ls = np.log(t) + a + np.log(-np.expm1(-2.0 * a)) - LN2
    ls[0] = NO_TERM
    lc = np.log(h) + (1.0 - nu) * np.log(2.0) - math.lgamma(nu)
    psi = digamma_host(nu)
    r = np.asarray(r, dtype=np.float64)
    rr = np.where(r == 0.0, 2.220446049250313e-16, r)
    s2nu = np.sqrt(2.0 * nu)
    x = np.minimum(np.maximum(rr * s2nu, gen_xmin64(nu, nodes)), 1.0e5)
    lx = np.log(x)
    mu = max(nu, 1.0 - nu)
    T = np.log(2.0 * (41.0 + mu * np.maximum(1.0, 4.40671924726425 - lx))) - lx
    N = np.minimum((np.maximum(T, 1.0) / h).astype(np.int64) + 3, nodes)
    if not truncate:
        N = np.full_like(N, nodes)
    L = nu * lx + lc
    s1 = np.zeros_like(x)
    s0 = np.zeros_like(x)
    sd = np.zeros_like(x)
    for i in range(int(N.max())):
        on = i < N
        base = x * negc[i] + L
        s1 = s1 + np.where(on, np.exp(base + l1[i]), 0.0)
        if want_nu:
            s0 = s0 + np.where(on, np.exp(base + l[i]), 0.0)
            sd = sd + np.where(on, np.exp(base + ls[i]), 0.0)
    zero = r == 0
    dr = np.where(zero, 0.0, -s2nu * s1)
    if not want_nu:
        return dr, None
    dnu = s0 * (lx - LN2 - psi) + sd - (x / (2.0 * nu)) * s1
    return dr, np.where(zero, 0.0, dnu)


def dk_dr_scipy(r, nu):
    """-sqrt(2 nu) c x^nu K_{nu-1}(x), zero where the Bessel function underflows."""
    from scipy.special import kv

    r = np.asarray(r, dtype=np.float64)
    x = np.sqrt(2.0 * nu) * r
    with np.errstate(all="ignore"):
        v = -np.sqrt(2.0 * nu) * np.exp((1.0 - nu) * np.log(2.0) - math.lgamma(nu) + nu * np.log(x)) * kv(nu - 1.0, x)
    return np.where(np.isfinite(v), v, 0.0)


def dk_dnu_richardson(r, nu, fn, h=None):
    """Richardson central difference (4 D(h / 2) - D(h)) / 3 of ``fn(r, nu)`` in nu."""
    h = (1e-3 * max(1.0, nu)) if h is None else h
    h = min(h, 0.5 * nu)

    def D(s):
        return (fn(r, nu + s) - fn(r, nu - s)) / (2.0 * s)

    return (4.0 * D(0.5 * h) - D(h)) / 3.0
