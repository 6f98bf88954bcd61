"""GPU: the wave-sized forward with a length scale per neighbourhood (mgp_posterior_ns_wave_*, ns_wave_forward_kernel)
against the fp64 reference of tests/nonstationary_cases.py at the edges of its instantiations, its task loop and
position independence, bad scales, and the ``fused.ns_forward("wave")`` ladder with the functor route on top of it.

The band is RTOL of tests/util.py (fp64 1e-5, fp32 1e-3): ``assert_close`` for the mean, the pure relative
``assert_rel_close`` for the variance and y^T K^-1 y -- what the LDS and slab NS kernels are held to on the same recipe.
Every case asserts the instantiation that served it by name and prints its figures before it asserts."""

import ctypes as C

import numpy as np
import pytest
import torch

from tests import nonstationary_cases as NC
from tests.posterior_cases import band_error, rel_error
from tests.util import RTOL, assert_close, assert_rel_close, to_dev

pytestmark = pytest.mark.gpu

TORCH = {"float32": torch.float32, "float64": torch.float64}
F32, F64 = "float32", "float64"


def _register(cases):
    for c in cases:
        NC.BY_ID.setdefault(c["id"], c)
    return [c["id"] for c in cases]


def _run(c, P, ls, name, rows=None, info=None):
    """One ``path="wave"`` launch of the case on neighbourhoods ``rows`` (default: all) with the (b, 1) scales ``ls``;
    ``name``: the (NP, DG) of the instantiation that must serve it.  Returns numpy (mean, var, ykinvy), (len(rows), -1) each."""
    from muygpys_amd import _lib
    from muygpys_amd.fused import KernelSpec, posterior_mean_var

    dt = TORCH[c["dtype"]]
    rows = np.arange(P.b) if rows is None else np.asarray(rows)
    noise = NC.NOISE if c["noise"] == "scalar" else to_dev(P.table if c["noise"] == "table" else P.noise_rows[rows], dt)
    spec = KernelSpec(c["kernel"], c["metric"], 1.0, noise, length_scale_batch=to_dev(np.ascontiguousarray(ls), dt))
    Xq = to_dev(P.Xq if c["bi"] else P.Xq[rows], dt)  # (no batch index: neighbourhood i reads query row i)
    bi = to_dev(P.bi[rows]) if c["bi"] else None
    tg = to_dev(P.Y[P.ni[rows]] if c["gathered"] else P.Y, dt)
    out = posterior_mean_var(spec, Xq, to_dev(P.Xn, dt), bi, to_dev(P.ni[rows]), tg, want_ykinvy=True, path="wave",
                             gathered=c["gathered"], info=info)
    torch.cuda.synchronize()
    want = "mgp::ns_wave_forward_kernel<{},{},{}>".format(NC.CNAME[c["dtype"]], *name)
    assert _lib.last_kernel() == want, (_lib.last_kernel(), want)
    return tuple(o.double().cpu().numpy().reshape(len(rows), -1) for o in out)


def _in_band(what, got, ref, rtol):
    (mean, var, yk), (m_ref, v_ref, y_ref) = got, ref
    print(f"FIGURES {what} mean {band_error(mean, m_ref) / rtol:.2e} var {rel_error(var.reshape(-1), v_ref) / rtol:.2e} "
          f"ykinvy {rel_error(yk, y_ref) / rtol:.2e} of the band")
    assert_close(mean, m_ref, rtol, f"{what}: mean")
    assert_rel_close(var.reshape(-1), v_ref, rtol, f"{what}: var")
    assert_rel_close(yk, y_ref, rtol, f"{what}: ykinvy")


# ---- 1. against the fp64 reference, at the edges --------------------------------------------------------------------------
_W = "wave"
EDGES = [
    (NC._case(_W, F32, 1, 1, b=1), (32, 4)),
    (NC._case(_W, F32, 30, 40, noise="table"), (32, 10)),
    (NC._case(_W, F32, 28, 8, R=3, kernel="rbf", metric="F2", gathered=True, noise="batch"), (32, 4)),
    (NC._case(_W, F32, 31, 3, bi=False), (64, 4)),
    (NC._case(_W, F32, 60, 64, R=3), (64, 16)),
    (NC._case(_W, F32, 10, 41), (32, 12)),
    (NC._case(_W, F64, 30, 16), (32, 8)),
    (NC._case(_W, F64, 50, 8), (64, 4)),
    (NC._case(_W, F64, 2, 3, R=3, noise="batch", gathered=True), (32, 4)),
]
# every closed-form kernel name KernelSpec and the oracle's Spec share, both metrics: the per-lane scale enters each formula
EDGES += [(NC._case(_W, F32, 5, 3, kernel=kern, metric=metric), (32, 4))
          for kern in ("rbf", "matern05", "matern15", "matern25", "maternInf") for metric in ("l2", "F2")]
NAME = dict(zip(_register([c for c, _ in EDGES]), [n for _, n in EDGES]))


# Matern-3/2 of the SQUARED distance is not positive definite: at k = 5, d = 3 two of the seven reference systems of this one
# case have a smallest eigenvalue of -0.014 and -0.047 and no posterior.  There, and in no other case, the neighbourhoods
# the fp64 reference finds indefinite must return NaN rows and count once each in info; the others meet the band.
NOT_SPD = NC._case(_W, F32, 5, 3, kernel="matern15", metric="F2")["id"]


@pytest.mark.parametrize("case_id", list(NAME))
def test_a_against_the_fp64_reference(case_id, monkeypatch):
    from muygpys_amd.config import config

    c, P = NC.BY_ID[case_id], NC.problem(case_id)
    if case_id != NOT_SPD:  # (a pivot failure raises LinAlgError here)
        return _in_band(case_id, _run(c, P, P.ls, NAME[case_id]), NC.reference(case_id), RTOL[c["dtype"]])
    Kin = NC.posterior_per_neighbourhood(c["kernel"], c["metric"], P.Xq, P.Xn, P.bi, P.ni, P.Y, P.ls, P.noise_rows)[3]
    spd = np.array([np.linalg.eigvalsh(K).min() > 0.0 for K in Kin])
    info = torch.zeros(1, dtype=torch.int32, device="cuda")
    monkeypatch.setattr(config.state, "check_spd", False)  # (look at info ourselves)
    got = _run(c, P, P.ls, NAME[case_id], info=info)
    assert int(info.item()) == int((~spd).sum()) == 2
    assert all(np.isnan(a[~spd]).all() for a in got)
    _in_band(case_id, tuple(a[spd] for a in got), tuple(r[spd] for r in NC.reference(case_id)), RTOL[c["dtype"]])


# ---- 2. the task loop, both halves of a wave, both parities of the prefetch -----------------------------------------------
LOOP = dict(zip(_register([NC._case(_W, F32, 5, 3), NC._case(_W, F64, 33, 3)]), [(32, 4), (64, 4)]))


@pytest.mark.parametrize("case_id", list(LOOP))
def test_b_task_loop_and_position_independence(case_id):
    from muygpys_amd import _lib

    c, P = NC.BY_ID[case_id], NC.problem(case_id)
    copies = 1201
    rows = np.tile(np.arange(P.b), copies)  # 7 distinct neighbourhoods, 8407 in all: both odd
    got = _run(c, P, P.ls[rows], LOOP[case_id], rows=rows)
    grid, lds = C.c_int64(0), C.c_int(0)
    assert _lib.load().mgp_last_launch_geometry(C.byref(grid), C.byref(lds)) == 0
    tasks = -(-len(rows) // (64 // LOOP[case_id][0]))
    assert tasks > grid.value, f"{tasks} tasks on {grid.value} workgroups: the prefetch across tasks is not exercised"
    for name, a in zip(("mean", "var", "ykinvy"), got):
        a = a.reshape(copies, P.b, -1)
        assert all(a[j].tobytes() == a[0].tobytes() for j in range(1, copies)), f"{case_id}: {name} depends on the position"
    _in_band(case_id, tuple(a[:P.b] for a in got), NC.reference(case_id), RTOL[c["dtype"]])


# ---- 3. a bad scale --------------------------------------------------------------------------------------------------------
BAD = _register([NC._case(_W, dt, 12, 3, b=5, R=3) for dt in (F32, F64)])


@pytest.mark.parametrize("bad", [0.0, -1.0, float("nan"), float("inf")], ids=["zero", "negative", "nan", "inf"])
@pytest.mark.parametrize("case_id", BAD)
def test_c_a_bad_scale_spoils_its_own_neighbourhood_alone(case_id, bad, monkeypatch):
    from muygpys_amd.config import config

    c, P = NC.BY_ID[case_id], NC.problem(case_id)
    clean = _run(c, P, P.ls, (32, 4))
    ls = np.array(P.ls)
    ls[2, 0] = bad
    info = torch.zeros(1, dtype=torch.int32, device="cuda")
    with monkeypatch.context() as mp:
        mp.setattr(config.state, "check_spd", False)  # (this launch: look at info ourselves)
        got = _run(c, P, ls, (32, 4), info=info)
    assert int(info.item()) == 1
    keep = [0, 1, 3, 4]  # (3 shares its wave with 2)
    for name, a, g in zip(("mean", "var", "ykinvy"), clean, got):
        assert np.isnan(g[2]).all(), f"{case_id}: {name} of the bad neighbourhood is {g[2]}"
        assert a[keep].tobytes() == g[keep].tobytes(), f"{case_id}: {name} of a clean neighbourhood changed"
    with pytest.raises(np.linalg.LinAlgError, match="length scale"):
        _run(c, P, ls, (32, 4))


# ---- 4. the ladder and the functor route -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, F64])
def test_d_ladder_under_the_mode(dtype):
    from muygpys_amd import _lib, fused

    dt, t = TORCH[dtype], NC.CNAME[dtype]
    rng = np.random.default_rng(11)
    n, d, b = 300, 2, 3
    X, y = to_dev(rng.uniform(size=(n, d)), dt), to_dev(rng.normal(size=n), dt)

    def call(k, count=1):
        ni = to_dev(np.stack([rng.choice(n, size=k, replace=False) for _ in range(b)]))
        spec = fused.KernelSpec("matern15", "l2", 1.0, 0.05, length_scale_batch=to_dev(NC.draw_scales(rng, b, count), dt))
        fused.posterior_mean_var(spec, X, X, to_dev(np.arange(b)), ni, y)
        torch.cuda.synchronize()
        return _lib.last_kernel()

    before = fused.ns_forward_default()
    with fused.ns_forward("wave"):
        assert fused.ns_forward_default() == "wave"
        assert call(10) == f"mgp::ns_wave_forward_kernel<{t},32,4>"
        assert call(10, count=d) == f"mgp::fused_generic_ns_kernel<{t}>"  # (b, d) scales
        assert call(63) == f"mgp::fused_generic_ns_kernel<{t}>"  # k + 1 + R = 65
    assert fused.ns_forward_default() == before


def test_e_functor_route_under_the_mode(monkeypatch):
    from muygpys_amd import _lib, fused
    from tests.test_gpu_nonstationary import _count_ns_launches, _optimiser_problem

    m, (y_b, y_nn, cross, pair), bf = _optimiser_problem()
    host = lambda t: t.double().cpu().numpy()  # noqa: E731

    def evaluate():
        Kin, Kc = m.kernel(pair, batch_features=bf), m.kernel(cross, batch_features=bf)
        mean, var = m.posterior_mean(Kin, Kc, y_nn), m.get_opt_var_fn()(Kin, Kc)
        return host(mean), host(var), _lib.last_kernel()

    mean0, var0, name0 = evaluate()
    assert name0 == "mgp::fused_generic_ns_kernel<double>"
    launches = _count_ns_launches(monkeypatch)
    with fused.ns_forward("wave"):
        mean1, var1, name1 = evaluate()
    assert len(launches) == 1, "mean and variance of one evaluation share one fused NS launch"
    assert name1 == "mgp::ns_wave_forward_kernel<double,32,4>"
    assert_close(mean1, mean0, RTOL[F64], "mean against the default route's")
    assert_rel_close(var1, var0, RTOL[F64], "variance against the default route's")
