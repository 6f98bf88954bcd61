"""CPU: the derivative evaluators of the general-smoothness Matern (csrc/mgp_wave_common.h: matern_gen_deriv_eval,
matern_gen_deriv_batch64) restated in numpy at their working precision (tests/gen_deriv_restatement.py), with the
node-count rule in place and every pair at its OWN node count (the fewest nodes the device can give it), against scipy:

* dk/dr  against -sqrt(2 nu) c x^nu K_{nu-1}(x) (scipy.special.kv);
* dk/dnu against a Richardson central difference of ``oracle.matern_gen_fn``;
* r in [1e-4, 20] log-spaced, nu in {0.3, 0.42, 0.8, 1, 2.2, 3.7, 8, 25}.

The bounds are twice the errors of the UNTRUNCATED tables measured when the feature was specified (fp64: dk/dr 7e-13,
1.5e-12 at nu = 2; dk/dnu 3e-11, the reference's own limit.  fp32: dk/dr 9e-6 at nu = 0.3, 1.1e-6 for 0.8 <= nu <= 9,
4.9e-6 at nu = 25; dk/dnu 7.6e-6 for nu <= 2, 2.1e-5 at nu = 3.7, 7.8e-5 at nu = 25), each nu taking the bound of the
bracket it falls in.  Measured maxima of the truncated rule on this grid (and equal to the whole table's to the digits
shown: the rule drops nothing that matters):

    nu      fp64 dk/dr   fp64 dk/dnu   fp32 dk/dr   fp32 dk/dnu
    0.3     6.9e-13      2.4e-11       9.7e-06      2.6e-06
    0.42    7.1e-14      7.1e-12       2.0e-06      2.8e-06
    0.8     1.0e-13      2.9e-11       2.0e-07      2.8e-06
    1       2.2e-13      7.0e-12       1.7e-07      4.0e-06
    2.2     1.1e-14      6.1e-12       2.3e-07      3.9e-06
    3.7     2.0e-13      2.7e-12       2.9e-07      1.2e-05
    8       1.4e-15      6.0e-13       7.2e-07      3.1e-05
    25      6.2e-15      9.4e-13       3.4e-06      1.2e-04

(max |dk/dnu| itself falls from 0.89 at nu = 0.3 to 3.6e-4 at nu = 25: in fp32 the nu-derivative is of the forward's
order up to nu ~ 4 and a large fraction of itself above -- the GPU tests assert fp32 grad_nu for nu <= 4 only.)"""

import numpy as np
import pytest

from oracle.muygps_oracle import matern_gen_fn
from tests import gen_deriv_restatement as G

NUS = [0.3, 0.42, 0.8, 1.0, 2.2, 3.7, 8.0, 25.0]
R = np.logspace(-4, np.log10(20.0), 400)


def _bound_dr32(nu):
    return 2 * (9e-6 if nu < 0.8 else (1.1e-6 if nu <= 9 else 4.9e-6))


def _bound_dnu32(nu):
    return 2 * (7.6e-6 if nu <= 2 else (2.1e-5 if nu <= 3.7 else 7.8e-5))


@pytest.fixture(scope="module")
def refs():
    out = {}
    for nu in NUS:
        dnu = G.dk_dnu_richardson(R, nu, matern_gen_fn)
        out[nu] = (G.dk_dr_scipy(R, nu), np.where(np.isfinite(dnu), dnu, 0.0))
    return out


@pytest.mark.parametrize("nu", NUS)
def test_fp64_evaluator_matches_scipy(nu, refs):
    dr, dnu = G.deriv_fp64(R, nu)
    e_r, e_nu = np.abs(dr - refs[nu][0]).max(), np.abs(dnu - refs[nu][1]).max()
    print(f"nu={nu}: fp64 dk/dr err {e_r:.2e}, dk/dnu err {e_nu:.2e}")
    assert e_r <= 2 * 7e-13, (nu, e_r)  # (nu = 2.0, the one value the whole table misses this at, is not on the grid)
    assert e_nu <= 2 * 3e-11, (nu, e_nu)
    # the length-scale-only instantiation returns the same dk/dr
    assert np.array_equal(G.deriv_fp64(R, nu, want_nu=False)[0], dr)


@pytest.mark.parametrize("nu", NUS)
def test_fp32_evaluator_matches_scipy(nu, refs):
    dr, dnu = G.deriv_fp32(R, nu)
    assert dr.dtype == np.float32 and dnu.dtype == np.float32
    e_r = np.abs(dr.astype(np.float64) - refs[nu][0]).max()
    e_nu = np.abs(dnu.astype(np.float64) - refs[nu][1]).max()
    print(f"nu={nu}: fp32 dk/dr err {e_r:.2e}, dk/dnu err {e_nu:.2e}")
    assert e_r <= _bound_dr32(nu), (nu, e_r)
    assert e_nu <= _bound_dnu32(nu), (nu, e_nu)
    assert np.array_equal(G.deriv_fp32(R, nu, want_nu=False)[0], dr)


@pytest.mark.parametrize("nu", NUS)
def test_node_count_rule_loses_nothing_against_the_whole_table(nu):
    """The rule covers the slowest-decaying weight -- exp(max(nu, 1 - nu) t): cosh((1 - nu) t) below nu = 1/2 -- so the
    truncated sums agree with the whole table's far inside the bounds above, with a fraction of the nodes where
    distances live."""
    for fn, tol in ((G.deriv_fp64, 1e-14), (G.deriv_fp32, 2e-7)):
        a, b = fn(R, nu, truncate=True), fn(R, nu, truncate=False)
        scale = max(1.0, float(np.abs(b[0]).max()))
        assert np.abs(a[0].astype(np.float64) - b[0]).max() <= tol * scale, (nu, fn.__name__)
        assert np.abs(a[1].astype(np.float64) - b[1]).max() <= tol * scale, (nu, fn.__name__)


@pytest.mark.parametrize("nu", NUS)
def test_zero_distance_contributes_nothing(nu):
    for fn in (G.deriv_fp64, G.deriv_fp32):
        dr, dnu = fn(np.zeros(3), nu)
        assert not dr.any() and not dnu.any()


def test_digamma_restatement_matches_scipy():
    from scipy.special import digamma

    for x in (0.01, 0.3, 0.42, 1.0, 2.2, 3.7, 8.0, 25.0, 30.0):
        assert abs(G.digamma_host(x) - digamma(x)) <= 1e-13 * max(1.0, abs(digamma(x))), x
