"""CPU: the fp64 numpy reference of tests/nonstationary_cases.py (the oracle's functions, one neighbourhood at a time,
each with its own scale) against fixtures written by the real reference's nonstationary model
(tests/golden/hier/hier_*.npz, generator tests/golden/make_golden_nonstationary.py) and, at a constant scale, against the
oracle's scalar pipeline; and that the case table covers what the issue lists."""

import json
import os

import numpy as np
import pytest

from oracle import muygps_oracle as orc
from tests import nonstationary_cases as NC

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hier")
FIXTURES = ("hier_rbf_F2", "hier_m15_l2")


def _load(name):
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    return g, json.loads(str(g["meta"]))


@pytest.mark.parametrize("name", FIXTURES)
def test_reference_against_the_real_reference(name):
    g, meta = _load(name)
    X, y, bi, ni = g["features"], g["targets"], g["batch_idx"], g["nn_idx"]
    assert (meta["N"], meta["d"], meta["k"], meta["b"], meta["knot_count"]) == (400, 2, 8, 50, 5)
    assert g["scales"].shape == (50,) and np.all(g["scales"] > 0)
    noise_rows = np.full(ni.shape, meta["noise"])
    mean, var, yk, Kin, Kc = NC.posterior_per_neighbourhood(meta["kernel"], meta["metric"], X, X, bi, ni, y, g["scales"][:, None],
                                                            noise_rows)
    np.testing.assert_allclose(Kin - meta["noise"] * np.eye(meta["k"]), g["Kin"], rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(Kc, g["Kcross"], rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(mean[:, 0], g["mean"], rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(var, g["var_unscaled"], rtol=1e-8, atol=1e-13)
    np.testing.assert_allclose(yk.sum() / (meta["b"] * meta["k"]), g["sigma_sq"][0], rtol=1e-10)
    # the fixture can tell per-neighbourhood scales from one scale: the mean of the scales misses by far
    flat = orc.posterior_mean_var(orc.Spec(meta["kernel"], meta["metric"], float(g["scales"].mean()), meta["noise"]), X, X, bi, ni, y)
    assert np.abs(flat[0] - g["mean"]).max() > 1e-3


@pytest.mark.parametrize("name", FIXTURES)
def test_objective_probes_are_the_reference_objective_modules(name):
    """Two knot-value vectors with the reference's own ``make_loo_crossval_fn`` values for lool and mse (the script says
    which module computed them); the GPU test compares the functor route against them."""
    g, meta = _load(name)
    assert g["obj_lool"].shape == g["obj_mse"].shape == (2,) and g["probes"].shape == (2, 5)
    assert np.all(np.isfinite(g["obj_lool"])) and np.all(g["obj_mse"] < 0)
    assert meta["objective"] == "reference objective module"


@pytest.mark.parametrize("kernel, metric", [("rbf", "F2"), ("matern15", "l2"), ("matern05", "F2")])
@pytest.mark.parametrize("aniso", [False, True])
def test_constant_scale_is_the_oracles_scalar_result(kernel, metric, aniso):
    rng = np.random.default_rng(3)
    n, d, k, b, R = 120, 3, 9, 11, 2
    X, Xq = rng.uniform(size=(n, d)), rng.uniform(size=(b, d))
    Y = rng.normal(size=(n, R))
    ni = np.stack([rng.choice(n, size=k, replace=False) for _ in range(b)])
    bi = rng.permutation(b)
    ls = np.array([0.7, 1.3, 0.4]) if aniso else 0.8
    rows = np.repeat(np.atleast_1d(ls)[None, :], b, axis=0)
    mean, var, _, _, _ = NC.posterior_per_neighbourhood(kernel, metric, Xq, X, bi, ni, Y, rows, np.full((b, k), 0.03))
    m_ref, v_ref = orc.posterior_mean_var(orc.Spec(kernel, metric, ls, 0.03), Xq, X, bi, ni, Y)
    np.testing.assert_allclose(mean, m_ref, rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(var, v_ref, rtol=1e-12, atol=1e-14)


def test_case_table_covers_the_listed_values():
    G = [c for c in NC.CASES if c["entry"] == "generic"]
    L = [c for c in NC.CASES if c["entry"] == "large"]
    assert 20 <= len(NC.CASES) <= 30
    for dt in ("float32", "float64"):
        ks = {c["k"] for c in G if c["dtype"] == dt}
        assert {NC.lds_max(dt, 1), NC.lds_max(dt, 3)} & ks, (dt, ks)
        assert any(c["k"] == NC.lds_max(dt, c["R"]) + 1 for c in L if c["dtype"] == dt)
    assert {1, 2, 31, 64, 65} <= {c["k"] for c in G} and 2 in {c["k"] for c in L}
    assert any(c["d"] == 20 and c["k"] == NC.lds_max(c["dtype"], c["R"]) for c in G)
    for cases in (G, L):
        assert {c["R"] for c in cases} == {1, 3}
        assert {c["aniso"] for c in cases} == {False, True}
        assert {c["metric"] for c in cases} == {"l2", "F2"} and len({c["kernel"] for c in cases}) == 2
        assert {c["bi"] for c in cases} == {False, True}
        assert {c["noise"] for c in cases} == {"scalar", "table", "batch"}
        assert {c["gathered"] for c in cases} == {False, True}
        assert {1, 7} <= {c["b"] for c in cases} and any(c["b"] > 4096 for c in cases)
    assert {1, 3, 8, 40} <= {c["d"] for c in NC.CASES}
    # scales spread over the whole range, different in every neighbourhood
    P = NC.problem(NC.CASES[2]["id"])
    assert P.ls.min() < 0.25 and P.ls.max() > 4.0 and len(np.unique(P.ls)) == P.ls.size
