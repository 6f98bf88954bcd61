"""GPU: the hyper-parameter backward of the general-smoothness Matern (csrc/mgp_backward_gen_large.hip:
``mgp_hyper_backward_gen_large_*``, the derivative evaluators of csrc/mgp_wave_common.h) against the fp64 reference of
tests/gen_backward_reference.py -- ``reference_partials`` of tests/test_gpu_large_backward.py restated with dk/dr from
scipy's Bessel function and dk/dnu from a Richardson difference of ``oracle.matern_gen_fn``; pinned to central
differences on the CPU in tests/test_gen_backward_reference_cpu.py -- through the C entry at every strip, block and
tile edge, against the closed-form entry at nu = 1/2, 3/2, 5/2, placement invariance bit for bit, failure semantics,
the top of the range, ``fused.loocv_value_and_grad`` / ``class_value_and_grad`` and the L-BFGS-B driver.

Inputs as in tests/test_gpu_large_backward.py, with two rules of their own.  The evaluators are accurate in ABSOLUTE
terms (1e-12 / 4e-6 of a covariance that is at most 1), so the inputs keep covariances away from zero: the length scale
grows with sqrt(d / 8) beyond eight features (at d = 70 and length scale 0.5 every covariance, and with it every
gradient, would lie below 1e-10).  And the F2 metric goes with nu <= 1/2 wherever a neighbourhood has more than two
points: k(r^2) is positive definite in every dimension only if k is completely monotone, which the Matern function is
for nu <= 1/2 alone (tests/test_gpu_large_backward.py pairs F2 with rbf and matern05 for the same reason) -- beyond
that the neighbourhoods are counted as non-SPD, as they should be.

Strip edges of the built kernel: a strip of phase 4 (and of the
covariance phase) is NT threads x 4 pairs in fp32, x 2 in fp64, NT = 256 up to k = 126 and 512 beyond: 1024 pairs in
fp32 (k = 44 has 990, k = 45 1035) and 512 in fp64 (k = 31: 496, k = 32: 528) -- the k edges the feature was specified
with.

Bands: fp64 1e-5 everywhere; fp32 3e-3 (the slab backward's) for grad_ls and grad_noise at every nu and for grad_nu at
nu <= 4.  Above that the fp32 evaluator's error of dk/dnu (3e-5 at nu = 8, 1.2e-4 at nu = 25:
tests/test_matern_gen_deriv_cpu.py) is a large fraction of the derivative itself (max |dk/dnu| = 3.5e-3 at nu = 8):
fp32 grad_nu is computed there and must be finite, its value is covered by the fp64 cases.

One fp32 case of the edge sample falls outside the 3e-3 band (FP32_CASE_BANDS): d = 1 under F2 at nu = 0.3, where the
scaled squared distances of neighbouring points on a line reach the evaluators' lower clamp on x (1e-6, the forward's)
and k(x) ~ 1 - c x^0.6 still moves by 2.5e-4 there.  Its band is twice the deviation that the numpy-float32 restatement
of covariances (tests/test_matern_gen_cpu.py) and derivatives (tests/gen_deriv_restatement.py) causes when pushed
through the fp64 reference formula on that case's own inputs, measured on the CPU: grad_ls 1.073e-3 (the kernel's own
error on the GPU: 1.077e-3, against rms(ref) 3.6e-2), grad_nu 6.429e-3 -- hence 2.146e-3 and 1.286e-2, absolute.  On
every other fp32 case the same measurement stays below a tenth of the 3e-3 band."""

import numpy as np
import pytest
import torch

from tests import gen_backward_reference as GR
from tests.test_gpu_large_backward import (GRAD_RTOL, LS, NUGGET, TORCH, _functor_problem, cotangents, length_scales,
                                           make_table, neighbourhoods)
from tests.test_gpu_large_backward import entry as closed_form_entry
from tests.util import RTOL, assert_close, to_dev

pytestmark = pytest.mark.gpu

NU32_LIMIT = 4.0  # fp32 grad_nu is asserted up to here


def scales(rng, d, aniso):
    """length_scales of tests/test_gpu_large_backward.py, grown with sqrt(d / 8) beyond eight features."""
    return length_scales(rng, d, aniso) * max(1.0, np.sqrt(d / 8.0))


ALL = ("ls", "noise", "nu")


def entry(dtype, X_d, bi_d, ni_d, Y_d, noise, nu, metric, ls, gm, gv, gyk, want=ALL, workspace=None, sentinel=0.0):
    """One ``mgp_hyper_backward_gen_large_*`` call.  Returns (grad_ls, grad_noise, grad_nu, info): the outputs
    pre-filled with ``sentinel``, None where not asked for."""
    from muygpys_amd import _lib

    t = TORCH[dtype]
    lib, P = _lib.load(), _lib.ptr
    b, k = ni_d.shape
    d, R = X_d.shape[1], Y_d.shape[1]
    ls_d = to_dev(np.atleast_1d(ls), t)
    mode = (0, noise, None) if isinstance(noise, float) else (1 if noise.ndim == 1 else 2, 0.0, P(noise))
    if workspace is None:
        workspace = torch.empty(lib.mgp_backward_large_workspace_bytes(X_d.element_size(), k, b), dtype=torch.uint8, device="cuda")
    g_l = torch.full((b, ls_d.numel()), sentinel, device="cuda", dtype=t) if "ls" in want else None
    g_n = torch.full((b, k), sentinel, device="cuda", dtype=t) if "noise" in want else None
    g_nu = torch.full((b,), sentinel, device="cuda", dtype=t) if "nu" in want else None
    info = torch.zeros(1, dtype=torch.int32, device="cuda")
    cot = [None if g is None else to_dev(g, t) for g in (gm, gv, gyk)]
    rc = _lib.fn("hyper_backward_gen_large", t)(P(X_d), d, P(bi_d), P(ni_d), b, k, P(Y_d), R, *mode, float(nu),
                                                {"l2": 0, "F2": 1}[metric], P(ls_d), ls_d.numel(), *[P(g) for g in cot],
                                                P(g_l), P(g_n), P(g_nu), P(info), P(workspace), workspace.numel(),
                                                _lib.stream_ptr())
    assert rc == 0, rc
    torch.cuda.synchronize()
    name = f"mgp::hyper_backward_gen_large_kernel<{'float' if dtype == 'float32' else 'double'}, {'true' if 'nu' in want else 'false'}>"
    assert _lib.last_kernel() == name, _lib.last_kernel()
    return g_l, g_n, g_nu, int(info.item())


# absolute bands of single fp32 cases: twice the deviation of the float32 restatement (the module docstring)
FP32_CASE_BANDS = {"k31-d1-nu0.3-F2-iso-table-nobi-posterior-ls+nu-float32": {"grad_ls": 2 * 1.073e-3, "grad_nu": 2 * 6.429e-3}}


def check_partials(got, ref, dtype, nu, what):
    for g, r, name in zip(got, ref, ("grad_ls", "grad_noise", "grad_nu")):
        if g is None:
            continue
        g = g.double().cpu().numpy()
        print(f"{what}: {name} max |err| {np.abs(g - r).max():.3e}, rms(ref) {np.sqrt(np.mean(r * r)):.3e}")
        assert np.isfinite(g).all(), (what, name)
        if name == "grad_nu" and dtype == "float32" and nu > NU32_LIMIT:
            continue  # (see the module docstring)
        if name in FP32_CASE_BANDS.get(what, {}):
            assert np.abs(g - r).max() <= FP32_CASE_BANDS[what][name], (what, name, np.abs(g - r).max())
            continue
        assert_close(g, r, GRAD_RTOL[dtype], f"{what}: {name}")


def _metric_id_matches():
    from muygpys_amd import _lib

    assert _lib.METRIC_IDS == {"l2": 0, "F2": 1}


# ---- 1. the entry against the reference: a spread sample over every axis -------------------------------------------------
EDGE_K = (1, 2, 31, 32, 44, 45, 126, 127, 140)
EDGE_D = (1, 3, 8, 70)
EDGE_NU = (0.3, 0.42, 1.0, 2.2, 3.7, 8.0)
FORMS = ("loocv", "posterior", "posterior3")
WANTS = tuple(tuple(n for i, n in enumerate(ALL) if (m >> i) & 1) for m in range(1, 8))


def _edge_cases():
    rng = np.random.default_rng(20261021)
    n_cases = 45

    def spread(values):
        reps = -(-n_cases // len(values))
        return [values[i] for i in rng.permutation(np.tile(np.arange(len(values)), reps))[:n_cases]]

    cols = dict(k=spread(EDGE_K), d=spread(EDGE_D), nu=spread(EDGE_NU), metric=spread(("l2", "F2")), aniso=spread((False, True)),
                noise=spread(("scalar", "table", "batch")), bi=spread((True, False)), dtype=spread(("float32", "float64")),
                form=spread(FORMS), want=spread(WANTS))
    cases = [{name: vals[i] for name, vals in cols.items()} for i in range(n_cases)]
    # ... and the combinations at which the kernel takes a path of its own: each strip edge in the width it belongs to
    # and either block size next to the switch in both widths, every output, per-feature scales over two feature
    # chunks, and nu below 1/2 (where the node count follows cosh((1 - nu) t)) in both widths
    forced = [(31, 3, "float64", 1.0), (32, 3, "float64", 0.42), (44, 8, "float32", 2.2), (45, 8, "float32", 0.3),
              (126, 8, "float32", 3.7), (127, 8, "float32", 1.0), (126, 3, "float64", 8.0), (127, 3, "float64", 0.3),
              (33, 70, "float32", 0.42), (33, 70, "float64", 2.2)]
    for j, (k, d, dtype, nu) in enumerate(forced):
        base = dict(cases[j])
        base.update(k=k, d=d, dtype=dtype, nu=nu, aniso=True, want=ALL)
        cases.append(base)
    # F2 with more than two points: nu <= 1/2 (the module docstring)
    low = 0
    for c in cases:
        if c["metric"] == "F2" and c["k"] > 2 and c["nu"] > 0.5:
            c["nu"] = (0.3, 0.42)[low % 2]
            low += 1
    return cases


EDGE_CASES = _edge_cases()


def _edge_id(c):
    return (f"k{c['k']}-d{c['d']}-nu{c['nu']}-{c['metric']}-{'aniso' if c['aniso'] else 'iso'}-{c['noise']}"
            f"-{'bi' if c['bi'] else 'nobi'}-{c['form']}-{'+'.join(c['want'])}-{c['dtype']}")


def test_edge_sample_covers_every_factor():
    seen = {name: {c[name] for c in EDGE_CASES} for name in EDGE_CASES[0]}
    assert seen["k"] >= set(EDGE_K) and seen["d"] == set(EDGE_D) and seen["nu"] == set(EDGE_NU)
    assert seen["metric"] == {"l2", "F2"} and seen["noise"] == {"scalar", "table", "batch"}
    assert seen["aniso"] == {False, True} and seen["bi"] == {False, True} and seen["form"] == set(FORMS)
    assert seen["want"] == set(WANTS) and len(WANTS) == 7 and seen["dtype"] == {"float32", "float64"}
    assert len(EDGE_CASES) <= 60 and set(FP32_CASE_BANDS) <= {_edge_id(c) for c in EDGE_CASES}
    _metric_id_matches()


def edge_problem(c):
    """The inputs of one edge case, on the host: (X, Y, bi, ni, ls, table, rows, (gm, gv, gyk))."""
    rng = np.random.default_rng(sum(map(ord, _edge_id(c))))
    k, d, b, n = c["k"], c["d"], 5, 300
    gm, gv, gyk, R = cotangents(rng, c["form"], b)
    X, Y = make_table(rng, n, d, R)
    ni = neighbourhoods(rng, n, b, k)
    bi = rng.choice(n, size=b, replace=False) if c["bi"] else np.arange(b)
    ls = scales(rng, d, c["aniso"])
    table = NUGGET * (1.0 + rng.uniform(size=n))
    rows = np.full((b, k), NUGGET) if c["noise"] == "scalar" else table[ni]
    return X, Y, bi, ni, ls, table, rows, (gm, gv, gyk)


@pytest.mark.parametrize("c", EDGE_CASES, ids=[_edge_id(c) for c in EDGE_CASES])
def test_strip_block_and_tile_edges(c):
    dtype, nu = c["dtype"], c["nu"]
    X, Y, bi, ni, ls, table, rows, cot = edge_problem(c)
    t = TORCH[dtype]
    noise = NUGGET if c["noise"] == "scalar" else to_dev(table if c["noise"] == "table" else rows, t)
    ref = GR.partials(X, bi, ni, Y, rows, nu, c["metric"], ls, *cot)
    *got, info = entry(dtype, to_dev(X, t), to_dev(bi) if c["bi"] else None, to_dev(ni), to_dev(Y, t), noise, nu,
                       c["metric"], ls, *cot, want=c["want"])
    assert info == 0
    assert [g is None for g in got] == [w not in c["want"] for w in ALL]
    check_partials(got, ref, dtype, nu, _edge_id(c))


# ---- 2. agreement with the closed forms: no oracle involved ------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("nu, kernel", [(0.5, "matern05"), (1.5, "matern15"), (2.5, "matern25")])
@pytest.mark.parametrize("aniso", [False, True])
def test_agrees_with_the_closed_form_entry(nu, kernel, aniso, dtype):
    rng = np.random.default_rng(int(10 * nu) + aniso)
    n, d, k, b = 400, 8, 70, 8
    X, Y = make_table(rng, n, d)
    ni, bi = neighbourhoods(rng, n, b, k), rng.choice(n, size=b, replace=False)
    ls = length_scales(rng, d, aniso)
    gm, gv, gyk, _ = cotangents(rng, "loocv", b)
    t = TORCH[dtype]
    args = (dtype, to_dev(X, t), to_dev(bi), to_dev(ni), to_dev(Y, t), NUGGET)
    c_l, c_n, bad = closed_form_entry(*args, kernel, "l2", ls, gm, gv, gyk)
    g_l, g_n, _, info = entry(*args, nu, "l2", ls, gm, gv, gyk)
    assert bad == 0 and info == 0
    check_partials((g_l, g_n), (c_l.double().cpu().numpy(), c_n.double().cpu().numpy()), dtype, nu, f"nu = {nu} vs {kernel}")


# ---- 3. placement invariance, bitwise ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_placement_invariance_bitwise(dtype):
    from muygpys_amd import _lib

    rng = np.random.default_rng(300)
    n, d, k, b = 600, 8, 150, 9
    X, Y = make_table(rng, n, d)
    ni, bi = neighbourhoods(rng, n, b, k), rng.choice(n, size=b, replace=False)
    ls = length_scales(rng, d, True)
    gm, gv, gyk, _ = cotangents(rng, "loocv", b)
    t = TORCH[dtype]
    Xd, Yd = to_dev(X, t), to_dev(Y, t)
    slab = _lib.load().mgp_backward_large_workspace_bytes(Xd.element_size(), k, 1)

    def run(rows, slabs=None):
        rows = np.asarray(rows)
        size = _lib.load().mgp_backward_large_workspace_bytes(Xd.element_size(), k, len(rows)) if slabs is None else slabs * slab
        ws = torch.empty(size, dtype=torch.uint8, device="cuda")
        ws.fill_(0xFF)  # (what the slab held before must not matter: NaN in every element, either width)
        *got, info = entry(dtype, Xd, to_dev(bi[rows]), to_dev(ni[rows]), Yd, NUGGET, 1.3, "l2", ls, gm[rows], gv[rows],
                           gyk[rows], workspace=ws)
        assert info == 0
        return [g.cpu().numpy() for g in got]

    alone = run([0])
    assert all(np.isfinite(a).all() for a in alone)
    for name, got, pos in (("first of 9", run([0, 1, 2, 3, 4, 5, 6, 7, 8]), 0), ("last of 9", run([1, 2, 3, 4, 5, 6, 7, 8, 0]), 8),
                           ("one slab", run([3, 4, 0, 5, 6], 1), 2), ("recommended", run([3, 4, 0, 5, 6]), 2)):
        for a, g, what in zip(alone, got, ("grad_ls", "grad_noise", "grad_nu")):
            assert a[0].tobytes() == g[pos].tobytes(), (name, what, a[0], g[pos])


# ---- 4. failure semantics, zero distances ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_singular_neighbourhoods_are_counted_and_left_untouched(dtype):
    rng = np.random.default_rng(6)
    n, d, k, b = 500, 8, 90, 8
    X, Y = make_table(rng, n, d)
    ni, bi = neighbourhoods(rng, n, b, k), rng.choice(n, size=b, replace=False)
    broken = np.array([2, 7])
    ni[broken, 1] = ni[broken, 0]  # a duplicated neighbour ...
    noise = np.full((b, k), NUGGET)
    noise[broken] = 0.0            # ... and no nugget: exactly singular
    good = np.setdiff1d(np.arange(b), broken)
    gm, gv, gyk, _ = cotangents(rng, "loocv", b)
    ref = GR.partials(X, bi[good], ni[good], Y, noise[good], 1.3, "l2", LS, gm[good], gv[good], gyk[good])
    t, sentinel = TORCH[dtype], -777.0
    *got, info = entry(dtype, to_dev(X, t), to_dev(bi), to_dev(ni), to_dev(Y, t), to_dev(noise, t), 1.3, "l2", LS,
                       gm, gv, gyk, sentinel=sentinel)
    assert info == 2
    assert all((g[to_dev(broken)] == sentinel).all() for g in got)
    check_partials([g[to_dev(good)] for g in got], ref, dtype, 1.3, "the six good neighbourhoods")


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("metric, aniso, nu", [("l2", False, 0.3), ("l2", True, 1.0), ("F2", True, 0.42), ("F2", False, 0.3)])
def test_duplicate_rows_give_finite_values_that_match_the_reference(metric, aniso, nu, dtype):
    """Pairs at zero distance (a neighbour twice, and the query among its neighbours) with a nugget: nothing of them
    reaches grad_ls or grad_nu, below nu = 1/2 -- where dk/dr diverges at 0 -- as elsewhere."""
    rng = np.random.default_rng(8)
    n, d, k, b = 300, 3, 40, 6
    X, Y = make_table(rng, n, d)
    ni, bi = neighbourhoods(rng, n, b, k), rng.choice(n, size=b, replace=False)
    ni[:, 1] = ni[:, 0]
    ni[::2, 5] = bi[::2]
    ls = length_scales(rng, d, aniso)
    gm, gv, gyk, _ = cotangents(rng, "loocv", b)
    rows = np.full((b, k), NUGGET)
    ref = GR.partials(X, bi, ni, Y, rows, nu, metric, ls, gm, gv, gyk)
    t = TORCH[dtype]
    *got, info = entry(dtype, to_dev(X, t), to_dev(bi), to_dev(ni), to_dev(Y, t), NUGGET, nu, metric, ls, gm, gv, gyk)
    assert info == 0
    check_partials(got, ref, dtype, nu, f"duplicates, {metric}, nu = {nu}")


# ---- 5. the top of the range -----------------------------------------------------------------------------------------------
_TOP = {}


def _top_problem():
    if not _TOP:
        from muygpys_amd import _lib

        k = min(_lib.load().mgp_backward_gen_large_max_nn_count(es) for es in (4, 8))
        rng = np.random.default_rng(1022)
        n, d, b = 1100, 4, 1
        X, Y = make_table(rng, n, d)
        ni, bi = neighbourhoods(rng, n, b, k), rng.choice(n, size=b, replace=False)
        gm, gv, gyk, _ = cotangents(rng, "loocv", b)
        ref = GR.partials(X, bi, ni, Y, np.full((b, k), NUGGET), 1.3, "l2", LS, gm, gv, gyk)
        _TOP.update(k=k, X=X, Y=Y, ni=ni, bi=bi, cot=(gm, gv, gyk), ref=ref)
    return _TOP


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_top_of_the_range(dtype):
    p = _top_problem()
    assert p["k"] == 1022
    t = TORCH[dtype]
    *got, info = entry(dtype, to_dev(p["X"], t), to_dev(p["bi"]), to_dev(p["ni"]), to_dev(p["Y"], t), NUGGET, 1.3, "l2", LS,
                       *p["cot"])
    assert info == 0
    check_partials(got, p["ref"], dtype, 1.3, f"k = {p['k']}")


# ---- 6. loocv_value_and_grad through the functor layer's objective ---------------------------------------------------------
def _gen_model(nu0, ls0, noise=1e-2, free_noise=False, scale=None, free_nu=True, free_ls=True):
    from muygpys_amd.gp import MuyGPS
    from muygpys_amd.gp.deformation import Isotropy, l2
    from muygpys_amd.gp.hyperparameter import AnalyticScale, Parameter
    from muygpys_amd.gp.kernels import Matern
    from muygpys_amd.gp.noise import HomoscedasticNoise

    nu = Parameter(float(nu0), (0.2, 5.0)) if free_nu else Parameter(float(nu0))
    ls = Parameter(float(ls0), (0.2, 20.0)) if free_ls else Parameter(float(ls0))
    return MuyGPS(kernel=Matern(smoothness=nu, deformation=Isotropy(l2, ls)),
                  noise=HomoscedasticNoise(noise, (1e-4, 1.0)) if free_noise else HomoscedasticNoise(noise),
                  scale=AnalyticScale() if scale is None else scale)


FUNCTOR_CASES = [("lool", "analytic1", False), ("lool", "analytic3", False), ("lool", "fixed", False), ("lool", "analytic1", True),
                 ("mse", "analytic1", False), ("pseudo_huber", "analytic1", False), ("looph", "analytic3", True),
                 ("looph", "analytic1", False)]


@pytest.mark.parametrize("k", [30, 63], ids=["k30", "k63-first-beyond-64-slots"])
@pytest.mark.parametrize("loss, scale_kind, free_noise", FUNCTOR_CASES,
                         ids=[f"{c[0]}-{c[1]}-{'split' if c[2] else 'one'}" for c in FUNCTOR_CASES])
def test_gradient_is_the_central_difference_of_the_functor_layers_objective(loss, scale_kind, free_noise, k):
    """fp64, every loss, the analytic scale with iteration_count 1 and 3, a fixed scale, the sigma_noise split (a free
    noise): length scale, noise and smoothness against central differences of the objective the drivers maximise --
    rtol = 2e-6, atol = 2e-7 max |fd|, as tests/test_gpu_large_backward.py."""
    from muygpys_amd import _lib
    from muygpys_amd import optimize as O
    from muygpys_amd._src.optimize.chassis.hip import _analytic_value_and_grad
    from muygpys_amd.gp.hyperparameter import AnalyticScale, FixedScale
    from muygpys_amd.optimize import L_BFGS_B_optimize

    d = 4
    X, y, bi, ni = _functor_problem(31 + k, 800, 48, k, d, np.full(d, 1.2))
    scale = {"analytic1": None, "analytic3": AnalyticScale(iteration_count=3, val=0.8), "fixed": FixedScale(val=0.37)}[scale_kind]
    m = _gen_model(1.3, 1.4, free_noise=free_noise, scale=scale)
    Xd, yd = to_dev(X, torch.float64), to_dev(y, torch.float64)
    cross, pair, y_b, y_nn = m.make_train_tensors(to_dev(bi), to_dev(ni), Xd, yd)
    obj = L_BFGS_B_optimize.make_obj_fn(m, y_b, y_nn, cross, pair, loss_fn=getattr(O.loss, loss + "_fn"))
    names, x0, _ = m.get_opt_params()
    assert "smoothness" in names and "length_scale" in names and ("noise" in names) == free_noise
    x0 = np.asarray(x0, dtype=np.float64)
    value, grad = _analytic_value_and_grad(m, obj, names)(x0)
    assert _lib.last_kernel() == "mgp::hyper_backward_gen_large_kernel<double, true>"
    f = lambda x: -float(obj(**{n_: float(v) for n_, v in zip(names, x)}))  # noqa: E731  (the minimised function)
    np.testing.assert_allclose(value, f(x0), rtol=1e-10)
    fd = np.zeros_like(x0)
    for j in range(x0.size):
        h = 1e-5 * max(1.0, abs(x0[j])) if names[j] != "noise" else 1e-3 * x0[j]
        e = np.zeros_like(x0)
        e[j] = h
        fd[j] = (f(x0 + e) - f(x0 - e)) / (2 * h)
    print(f"{names}: analytic {grad!r} against central difference {fd!r}")
    np.testing.assert_allclose(grad, fd, rtol=2e-6, atol=2e-7 * np.abs(fd).max())


def test_a_fixed_smoothness_off_the_closed_forms_simply_works():
    """nu = 2.0 fixed, length scale and noise free: the general-nu kernels serve forward and backward, no grad_nu."""
    from muygpys_amd import _lib
    from muygpys_amd._src.optimize.chassis.hip import _analytic_value_and_grad
    from muygpys_amd.optimize import L_BFGS_B_optimize

    d, k = 4, 30
    X, y, bi, ni = _functor_problem(77, 800, 48, k, d, np.full(d, 1.2))
    m = _gen_model(2.0, 1.4, free_noise=True, free_nu=False)
    cross, pair, y_b, y_nn = m.make_train_tensors(to_dev(bi), to_dev(ni), to_dev(X, torch.float64), to_dev(y, torch.float64))
    obj = L_BFGS_B_optimize.make_obj_fn(m, y_b, y_nn, cross, pair)
    names, x0, _ = m.get_opt_params()
    assert "smoothness" not in names
    x0 = np.asarray(x0, dtype=np.float64)
    value, grad = _analytic_value_and_grad(m, obj, names)(x0)
    assert _lib.last_kernel() == "mgp::hyper_backward_gen_large_kernel<double, false>"
    f = lambda x: -float(obj(**{n_: float(v) for n_, v in zip(names, x)}))  # noqa: E731
    fd = np.zeros_like(x0)
    for j in range(x0.size):
        h = 1e-5 * max(1.0, abs(x0[j])) if names[j] != "noise" else 1e-3 * x0[j]
        e = np.zeros_like(x0)
        e[j] = h
        fd[j] = (f(x0 + e) - f(x0 - e)) / (2 * h)
    np.testing.assert_allclose(value, f(x0), rtol=1e-10)
    np.testing.assert_allclose(grad, fd, rtol=2e-6, atol=2e-7 * np.abs(fd).max())


def test_a_trial_smoothness_on_a_closed_form_keeps_the_general_form():
    """A free nu that sits exactly on 3/2: the evaluation stays on the general form, whose grad_nu exists."""
    from muygpys_amd import _lib
    from muygpys_amd._src.optimize.chassis.hip import _analytic_value_and_grad
    from muygpys_amd.optimize import L_BFGS_B_optimize

    d, k = 4, 30
    X, y, bi, ni = _functor_problem(78, 800, 48, k, d, np.full(d, 1.2))
    m = _gen_model(1.5, 1.4)
    cross, pair, y_b, y_nn = m.make_train_tensors(to_dev(bi), to_dev(ni), to_dev(X, torch.float64), to_dev(y, torch.float64))
    obj = L_BFGS_B_optimize.make_obj_fn(m, y_b, y_nn, cross, pair)
    names, x0, _ = m.get_opt_params()
    x0 = np.asarray(x0, dtype=np.float64)
    value, grad = _analytic_value_and_grad(m, obj, names)(x0)
    assert _lib.last_kernel() == "mgp::hyper_backward_gen_large_kernel<double, true>"
    f = lambda x: -float(obj(**{n_: float(v) for n_, v in zip(names, x)}))  # noqa: E731
    j = list(names).index("smoothness")
    e = np.zeros_like(x0)
    e[j] = 1e-5
    fd = (f(x0 + e) - f(x0 - e)) / 2e-5
    np.testing.assert_allclose(value, f(x0), rtol=1e-9)
    np.testing.assert_allclose(grad[j], fd, rtol=2e-6, atol=2e-7 * abs(fd))


# ---- 7. class_value_and_grad -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss", ["cross_entropy", "mse"])
def test_classification_gradient(loss):
    """Three one-hot columns, fp64, k = 70: value and gradient (length scale, noise, nu) against central differences of
    the function's own value -- and the mse case against the reference's partials."""
    from muygpys_amd import _lib, fused

    rng = np.random.default_rng(73)
    n, d, R, k, b = 700, 4, 3, 70, 12
    nu = 1.3
    X = rng.uniform(size=(n, d))
    labels = np.eye(R)[(np.floor(3.0 * X[:, :2].sum(1)) % R).astype(int)]
    ni, bi = neighbourhoods(rng, n, b, k), rng.choice(n, size=b, replace=False)
    t = torch.float64
    args = (to_dev(X, t), to_dev(labels, t), to_dev(bi), to_dev(ni))

    def run(ls=LS, noise=NUGGET, nu_=nu, **kw):
        return fused.class_value_and_grad(fused.KernelSpec("matern_gen", "l2", ls, noise, smoothness=nu_), *args, loss=loss, **kw)

    value, g_ls, g_noise, g_nu = run(grad_smoothness=True)
    assert _lib.last_kernel() == "mgp::hyper_backward_gen_large_kernel<double, true>"
    three = run()
    assert len(three) == 3 and three[0] == value
    h = 1e-6
    fd = [(run(ls=LS + h)[0] - run(ls=LS - h)[0]) / (2 * h), (run(noise=NUGGET + h)[0] - run(noise=NUGGET - h)[0]) / (2 * h),
          (run(nu_=nu + 1e-5)[0] - run(nu_=nu - 1e-5)[0]) / 2e-5]
    print(f"{loss}: analytic {(g_ls, g_noise, g_nu)!r} against central differences {fd!r}")
    np.testing.assert_allclose([g_ls[0], g_noise, g_nu], fd, rtol=2e-5, atol=2e-6 * np.abs(fd).max())
    if loss == "mse":
        rows = np.full((b, k), NUGGET)
        r = GR.outputs(X, bi, ni, labels, rows, nu, "l2", LS)[0] - labels[bi]
        p_ls, p_n, p_nu = GR.partials(X, bi, ni, labels, rows, nu, "l2", LS, 2.0 * r / (b * R), None, None)
        assert_close([value], [(r * r).sum() / (b * R)], RTOL["float64"], "mse value")
        assert_close(g_ls, p_ls.sum(0), GRAD_RTOL["float64"], "d / d length scale")
        assert_close([g_noise], [p_n.sum()], GRAD_RTOL["float64"], "d / d noise")
        assert_close([g_nu], [p_nu.sum()], GRAD_RTOL["float64"], "d / d nu")


# ---- 8. the driver -----------------------------------------------------------------------------------------------------
def test_lbfgsb_with_a_free_smoothness(monkeypatch):
    """fp64, a planted problem, nu and the length scale free: the analytic and the finite-difference driver end at the
    same point (1e-4 relative), and every analytic evaluation is one forward and one general-nu backward launch."""
    from muygpys_amd import _lib
    from muygpys_amd import fused as F
    from muygpys_amd.optimize import L_BFGS_B_optimize

    k, d = 30, 3
    X, y, bi, ni = _functor_problem(4, 2000, 150, k, d, np.full(d, 1.1))
    Xd, yd = to_dev(X, torch.float64), to_dev(y, torch.float64)
    calls = {"fwd": 0, "bwd": 0, "evals": 0}
    kernels = set()

    def counted(fn, key):
        def wrapper(*a, **kw):
            calls[key] += 1
            out = fn(*a, **kw)
            if key == "bwd":
                kernels.add(_lib.last_kernel())
            return out
        return wrapper

    for name, key in (("posterior_mean_var", "fwd"), ("loocv_partials", "fwd"), ("_hyper_partials", "bwd"),
                      ("loocv_value_and_grad", "evals")):
        monkeypatch.setattr(F, name, counted(getattr(F, name), key))
    results = {}
    for analytic in (False, True):
        m = _gen_model(1.0, 2.0, noise=1e-3)
        cross, pair, y_b, y_nn = m.make_train_tensors(to_dev(bi), to_dev(ni), Xd, yd)
        calls.update(fwd=0, bwd=0, evals=0)
        new = L_BFGS_B_optimize(m, y_b, y_nn, cross, pair, analytic_gradient=analytic)
        results[analytic] = (float(new.kernel.deformation.length_scale()), float(new.kernel.smoothness()), dict(calls))
    (ls_fd, nu_fd, n_fd), (ls_an, nu_an, n_an) = results[False], results[True]
    print(f"(length scale, nu) = {(ls_an, nu_an)!r} in {n_an} (analytic) against {(ls_fd, nu_fd)!r} in {n_fd} (finite differences)")
    assert n_fd["bwd"] == 0 and n_an["evals"] > 0 and n_an["fwd"] == n_an["evals"] and n_an["bwd"] == n_an["evals"]
    assert kernels == {"mgp::hyper_backward_gen_large_kernel<double, true>"}
    np.testing.assert_allclose([ls_an, nu_an], [ls_fd, nu_fd], rtol=1e-4)
    assert n_an["fwd"] < n_fd["fwd"], (n_an, n_fd)


# ---- 9. refusals ---------------------------------------------------------------------------------------------------------
def test_smoothness_bounds_beyond_the_kernel_are_a_named_error():
    from muygpys_amd.gp import MuyGPS
    from muygpys_amd.gp.deformation import Isotropy, l2
    from muygpys_amd.gp.hyperparameter import AnalyticScale, Parameter
    from muygpys_amd.gp.kernels import Matern
    from muygpys_amd.gp.noise import HomoscedasticNoise
    from muygpys_amd.optimize import L_BFGS_B_optimize

    X, y, bi, ni = _functor_problem(5, 300, 8, 10, 3, np.full(3, 1.1))
    m = MuyGPS(kernel=Matern(smoothness=Parameter(1.0, (0.5, 40.0)), deformation=Isotropy(l2, Parameter(1.0, (0.2, 20.0)))),
               noise=HomoscedasticNoise(1e-2), scale=AnalyticScale())
    cross, pair, y_b, y_nn = m.make_train_tensors(to_dev(bi), to_dev(ni), to_dev(X, torch.float64), to_dev(y, torch.float64))
    with pytest.raises(ValueError, match=r"\(0, 30\]"):
        L_BFGS_B_optimize(m, y_b, y_nn, cross, pair, analytic_gradient=True)


def test_grad_smoothness_of_a_closed_form_is_refused():
    from muygpys_amd import fused

    X, y, bi, ni = _functor_problem(5, 300, 8, 10, 3, np.full(3, 1.1))
    t = torch.float64
    with pytest.raises(ValueError, match="fixed smoothness"):
        fused.loocv_value_and_grad(fused.KernelSpec("matern15", "l2", 1.0, 1e-2), to_dev(X, t), to_dev(y, t), to_dev(bi),
                                   to_dev(ni), grad_smoothness=True)
