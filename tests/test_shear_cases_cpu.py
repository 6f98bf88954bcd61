"""What tests/test_gpu_shear_shapes.py relies on, asserted with the numpy oracle alone (no GPU, no library): the
problems of tests/shear_cases.py are well conditioned and strongly coupled at every neighbour count of the sweep, the
calibration function restates the oracle, and plain fp32 arithmetic stays inside the project's fp32 bound on them."""

import numpy as np
import pytest

from tests import shear_cases as S
from tests import shear_oracle as O

CASES = sorted(set(S.sweep("float64")) | set(S.sweep("float32")))


def test_problem_is_the_seeded_jittered_grid():
    P = S.problem()
    assert P.X.shape == (576, 2) and P.Y.shape == (576, 3) and P.Q.shape == (576, 2) and P.FQ.shape == (1152, 2)
    grid = np.stack(np.meshgrid(np.arange(24.0), np.arange(24.0), indexing="ij"), -1).reshape(-1, 2)
    assert np.abs(P.X - grid).max() <= 0.3 and np.abs(P.Q - grid - 0.5).max() <= 0.3
    assert not np.array_equal(P.X - grid, P.Q - grid - 0.5), "the query table has jitter of its own"
    # true nearest neighbours, the row itself excluded for a query from the table
    d2 = ((P.FQ[:, None, :] - P.X[None, :, :]) ** 2).sum(-1)
    rows = np.arange(len(P.FQ))[:, None]
    assert np.all(np.diff(d2[rows, P.order[:, :137]], axis=1) >= 0)
    assert np.all(P.order[:576, :575] != np.arange(576)[:, None])
    assert np.all(d2[rows, P.order[:, :137]].max(axis=1) <= np.partition(d2, 137, axis=1)[:, 137])


def test_sweep_reaches_every_shape_edge():
    for dtype in ("float64", "float32"):
        for i in (3, 2):
            ks = S.nn_counts(dtype, i)
            assert {(i * k) % 4 for k in ks} == {0, 1, 2, 3} if i == 3 else {(i * k) % 4 for k in ks} == {0, 2}
            assert any(i * k < 4 for k in ks)
            # both sides of the 64 / 256-thread switch (rows = n + 4 <= 64)
            assert any(i * k + 4 == 64 for k in ks) and any(64 < i * k + 4 <= 64 + i for k in ks)
            assert max(ks) == S.LIMIT[dtype, i] and set(S.PAIR_64K[dtype, i]) <= set(ks)


@pytest.mark.parametrize("in_count,mode,k,b", CASES)
def test_case_conditions_and_fp32_calibration(in_count, mode, k, b):
    c = S.case(in_count, mode, k, b, stats=True)
    assert c.bi.shape == (b,) and c.nn.shape == (b, k) and c.nn.max() < len(c.X)
    if b >= 37:
        assert (c.bi < 576).any() and (c.bi >= 576).any() and not np.array_equal(c.bi, np.arange(b))
    cond, ratio, ratio_cross = c.stats
    print(f"in={in_count} {mode} k={k} b={b}: cond {cond:.1f}, off-diag {ratio:.3f} (with Kcross {ratio_cross:.3f}), "
          f"smallest variance {np.diagonal(c.kout - c.kk, axis1=1, axis2=2).min():.2e}")
    assert cond <= 1e3
    if b >= 37:  # (a b = 1 case is one more system of a (model, noise mode, k) that has a b = 37 case)
        assert (ratio if k > 1 else ratio_cross) >= 0.5
    assert np.diagonal(c.kout - c.kk, axis1=1, axis2=2).min() > 0
    # the calibration restates the oracle (one chunk of systems says so as well as 300 do) ...
    h = min(b, 64) if k > 3 else b
    got = S.posterior_in_dtype(c.FQ, c.X, c.Y, c.bi[:h], c.nn[:h], c.ell, c.eps, in_count, mode, np.float64)
    for g, r, what in zip(got, (c.mean, c.kk, c.ykinvy), ("mean", "kk", "ykinvy")):
        assert S.metric_error(g, r[:h]) <= 1e-10, (what, S.metric_error(g, r[:h]))
    # ... and in fp32 stays inside the project's fp32 bound
    e = S.calibration(in_count, mode, k, b)
    print("fp32 calibration error (mean, kk, ykinvy)", e)
    assert max(e) <= 1e-3


@pytest.mark.parametrize("in_count,mode", [(3, "shear33"), (2, "homoscedastic")])
def test_zero_noise_case_stays_well_conditioned(in_count, mode):
    """The not-positive-definite test runs without a nugget: its healthy rows are still held to the tight bounds."""
    c = S.case(in_count, mode, 3, S.REUSE_B, 0.0, stats=True)
    assert c.stats[0] <= 1e3 and c.stats[1] >= 0.5
    got = S.posterior_in_dtype(c.FQ, c.X, c.Y, c.bi, c.nn, c.ell, 0.0, in_count, mode, np.float32)
    assert max(S.metric_error(g, r) for g, r in zip(got, (c.mean, c.kk, c.ykinvy))) <= 1e-3


def test_block_restatement_matches_the_oracle_block():
    rng = np.random.default_rng(S.SEED)
    d = rng.uniform(-2.8, 2.8, (500, 2))
    ref = O.block(d[:, 0], d[:, 1], 1.3)
    assert S.metric_error(S.block_in_dtype(d[:, 0], d[:, 1], 1.3, np.float64), ref) <= 1e-14
    assert S.block_in_dtype(d[:, 0], d[:, 1], 1.3, np.float32).dtype == np.float32
    assert S.metric_error(S.block_in_dtype(d[:, 0], d[:, 1], 1.3, np.float32), ref) <= 1e-5


@pytest.mark.parametrize("n,m,R", [(1, 1, 0), (7, 5, 4), (61, 3, 1), (276, 3, 1)])
def test_spd_systems_are_well_conditioned_and_restated(n, m, R):
    s = S.spd_systems(37 if n < 100 else 8, n, m, R, 0)
    w = np.linalg.eigvalsh(s.K)
    assert (w[:, -1] / w[:, 0]).max() <= 64
    for dtype, tol in ((np.float64, 1e-12), (np.float32, 1e-3)):
        got = S.solve_in_dtype(s.K, s.Kc, s.Y, dtype)
        for g, r in zip(got, (s.mean, s.kk, s.ykinvy)):
            assert S.metric_error(g, r) <= tol


def test_metric_error_is_the_project_metric():
    from tests.util import assert_close

    ref = np.array([1.0, -2.0, 0.0, 4.0])
    got = ref + np.array([1e-3, 0.0, 2e-3, -1e-3])
    t = S.metric_error(got, ref)
    assert_close(got, ref, t * (1 + 1e-12))
    with pytest.raises(AssertionError):
        assert_close(got, ref, t * (1 - 1e-6))
    assert S.metric_error(np.array([np.nan]), np.array([1.0])) == np.inf
