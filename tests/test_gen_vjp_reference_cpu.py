"""CPU: the fp64 reference of the feature and response cotangents of the general-smoothness Matern
(tests/gen_vjp_reference.py) is pinned to central differences of ``gen_backward_reference.outputs`` contracted with
random cotangents, sum_i gm_i . mean_i + gv_i var_i (+ gyk_i ykinvy_i): entries of the query table, of the neighbour
table and of the responses -- on either side of nu = 1/2 and of 1, under l2 and F2 (F2 with nu <= 1/2 alone: beyond it
k(r^2) is not positive definite, tests/test_gpu_gen_backward.py), Isotropy and Anisotropy, one and three responses and
the LOOCV form, two tables and one, and with a neighbour that appears twice (a table row behind two slots moves both:
the pair at zero distance stays at zero and must contribute nothing)."""

import numpy as np
import pytest

from tests import gen_vjp_reference as VR

FORMS = ("posterior", "posterior3", "loocv")


def _cotangents(rng, form, b):
    if form == "loocv":
        return rng.normal(size=b), rng.normal(size=b), rng.normal(size=b), 1
    if form == "posterior":
        return rng.normal(size=(b, 1)), rng.normal(size=b), None, 1
    return rng.normal(size=(b, 3)), None, None, 3


@pytest.mark.parametrize("shared", [False, True], ids=["two-tables", "one-table"])
@pytest.mark.parametrize("duplicate", [False, True], ids=["distinct", "duplicate"])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("aniso", [False, True], ids=["iso", "aniso"])
@pytest.mark.parametrize("nu, metric", [(0.42, "l2"), (0.42, "F2"), (1.3, "l2"), (3.7, "l2")])
def test_reference_vjp_is_the_central_difference(nu, metric, aniso, form, duplicate, shared):
    rng = np.random.default_rng(11)
    n, nq, d, b, k = 40, 9, 3, 3, 6
    gm, gv, gyk, R = _cotangents(rng, form, b)
    Xn = rng.uniform(size=(n, d))
    Xq = Xn if shared else rng.uniform(size=(nq, d))
    Y = np.stack([np.sin(3.0 * Xn.sum(1) + r) + 0.1 * rng.normal(size=n) for r in range(R)], axis=1)
    ni = np.stack([rng.choice(n, size=k, replace=False) for _ in range(b)])
    if duplicate:
        ni[:, 1] = ni[:, 0]
    bi = rng.choice(len(Xq), size=b, replace=False)
    ls = 0.5 * rng.uniform(0.7, 1.5, size=d) if aniso else np.array([0.5])
    rows = np.full((b, k), 1e-2)
    g_q, g_nn, g_t = VR.vjp(Xq, Xn, bi, ni, Y, rows, nu, metric, ls, gm, gv, gyk)

    def value(Xq_, Xn_, Y_):
        m, v, yk = VR.outputs(Xq_, Xn_, bi, ni, Y_, rows, nu, metric, ls)
        s = (np.reshape(gm, (b, R)) * m).sum() if gm is not None else 0.0
        s += (gv * v).sum() if gv is not None else 0.0
        s += (gyk * yk[:, 0]).sum() if gyk is not None else 0.0
        return s

    def fd(which, r, c, h=1e-6):
        def shifted(s):
            Xq_ = Xq.copy()
            Xn_ = Xq_ if shared else Xn.copy()  # (one table stays one table: both roles move)
            Y_ = Y.copy()
            (Xq_, Xn_, Y_)[which][r, c] += s
            return value(Xq_, Xn_, Y_)

        return (shifted(h) - shifted(-h)) / (2 * h)

    scale = max(np.abs(g_nn).max(), np.abs(g_q).max())
    untouched = np.setdiff1d(np.arange(n), np.append(ni.reshape(-1), bi if shared else []))[0]
    nn_rows = [ni[0, 0], ni[1, 1], ni[2, k - 1], untouched]
    for r in nn_rows:
        for c in (0, d - 1):
            want = g_nn[r, c] + (g_q[r, c] if shared else 0.0)
            np.testing.assert_allclose(want, fd(1, r, c), rtol=2e-6, atol=1e-7 * max(1.0, scale), err_msg=f"neighbour row {r}")
    for i in range(b):
        for c in (0, d - 1):
            want = g_q[bi[i], c] + (g_nn[bi[i], c] if shared else 0.0)
            np.testing.assert_allclose(want, fd(0, bi[i], c), rtol=2e-6, atol=1e-7 * max(1.0, scale), err_msg=f"query row {bi[i]}")
    assert (g_nn[untouched] == 0).all() and (g_t[untouched] == 0).all()
    for r in (ni[0, 0], ni[1, 2], ni[2, k - 1]):
        for q in range(R):
            np.testing.assert_allclose(g_t[r, q], fd(2, r, q), rtol=2e-6, atol=1e-7 * max(1.0, np.abs(g_t).max()),
                                       err_msg=f"response {r}, {q}")
    # only rows that a neighbourhood reads receive anything
    assert set(np.flatnonzero(np.abs(g_q).sum(1))) <= set(bi.tolist())
    assert set(np.flatnonzero(np.abs(g_nn).sum(1))) <= set(ni.reshape(-1).tolist())
