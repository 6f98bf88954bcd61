"""CPU: the fp64 reference the GPU tests of the general-smoothness backward compare against
(tests/gen_backward_reference.py) is itself pinned to central differences of its own forward outputs,
sum_i gm_i mean_i + gv_i var_i + gyk_i ykinvy_i, per neighbourhood: length scale(s), nugget and smoothness, both
metrics, Isotropy and Anisotropy, one smoothness on either side of 1/2 and of 1."""

import numpy as np
import pytest

from tests import gen_backward_reference as GR


@pytest.mark.parametrize("aniso", [False, True])
@pytest.mark.parametrize("nu, metric", [(0.3, "l2"), (0.42, "F2"), (1.0, "l2"), (2.2, "F2"), (3.7, "l2")])
def test_reference_partials_are_central_differences(nu, metric, aniso):
    rng = np.random.default_rng(5)
    n, d, b, k = 60, 3, 3, 6
    X = rng.uniform(size=(n, d))
    Y = np.sin(3.0 * X.sum(1))[:, None] + 0.1 * rng.normal(size=(n, 1))
    ni = np.stack([rng.choice(n, size=k, replace=False) for _ in range(b)])
    bi = rng.choice(n, size=b, replace=False)
    ls = 0.5 * rng.uniform(0.7, 1.5, size=d) if aniso else np.array([0.5])
    rows = np.full((b, k), 1e-2)
    gm, gv, gyk = rng.normal(size=b), rng.normal(size=b), rng.normal(size=b)
    g_ls, g_n, g_nu = GR.partials(X, bi, ni, Y, rows, nu, metric, ls, gm, gv, gyk)

    def value(ls_=ls, rows_=rows, nu_=nu):
        m, v, yk = GR.outputs(X, bi, ni, Y, rows_, nu_, metric, ls_)
        return gm * m[:, 0] + gv * v + gyk * yk[:, 0]

    h = 1e-6
    for c in range(ls.size):
        e = np.zeros(ls.size)
        e[c] = h
        np.testing.assert_allclose(g_ls[:, c], (value(ls_=ls + e) - value(ls_=ls - e)) / (2 * h), rtol=2e-6, atol=1e-7)
    for r in (0, k - 1):
        e = np.zeros((b, k))
        e[:, r] = h
        np.testing.assert_allclose(g_n[:, r], (value(rows_=rows + e) - value(rows_=rows - e)) / (2 * h), rtol=2e-6, atol=1e-7)
    hn = 1e-5
    np.testing.assert_allclose(g_nu, (value(nu_=nu + hn) - value(nu_=nu - hn)) / (2 * hn), rtol=2e-6, atol=1e-7)
