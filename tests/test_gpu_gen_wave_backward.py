"""GPU: the wave-sized hyper-parameter backward of the general-smoothness Matern (csrc/mgp_backward_wave_gen.h,
``mgp_hyper_backward_gen_wave_*``) against the fp64 reference of tests/gen_backward_reference.py at the edges of this
kernel -- the 32 / 64 slot switch (k = 30 / 31), the last slot count (62), an odd batch (a dead half-wave), the steps
of the row width, nu below 1/2 and at 1 -- then placement bit for bit (a partner with a far larger node count in the
same wave), failure and zero-distance semantics, and the ``"wavefront"`` switch of ``fused``.

Bands and input rules are those of tests/test_gpu_gen_backward.py (its docstring): fp64 1e-5, fp32 3e-3, fp32 grad_nu
asserted up to nu = 4 and finite beyond, F2 with nu <= 1/2 only, d = 1 kept away from F2 in fp32.

d = 1 is paired with fp32 at k = 2 only, and with fp64 at k = 30.  With 62 neighbours on a line at nu = 3.7 the fp32
EVALUATOR's error of dk/dnu, summed over 1953 pairs, leaves the 3e-3 band: measured on that input (5 neighbourhoods of
300 points), grad_nu of this kernel and of the slab kernel ``mgp_hyper_backward_gen_large_f32`` deviate from the fp64
reference by the same 4.888e-05 (identical to the last digit; rms(ref) 7.13e-03, band 2.1e-05 + 3e-3 |ref|), while
both fp64 kernels agree with it to 1e-10 -- the arithmetic the two kernels share, not this kernel's assembly of it."""

import numpy as np
import pytest
import torch

from tests import gen_backward_reference as GR
from tests.test_gpu_gen_backward import check_partials, scales
from tests.test_gpu_large_backward import NUGGET, TORCH, _functor_problem, cotangents, length_scales, make_table, neighbourhoods
from tests.util import to_dev

pytestmark = pytest.mark.gpu

OK, EUNSUPPORTED = 0, -2
ALL = ("ls", "noise", "nu")
NAME = "mgp::gen_wave_backward_kernel<"


def entry(dtype, X_d, bi_d, ni_d, Y_d, noise, nu, metric, ls, gm, gv, gyk, want=ALL, sentinel=0.0):
    """One ``mgp_hyper_backward_gen_wave_*`` call: (status, grad_ls, grad_noise, grad_nu, info)."""
    from muygpys_amd import _lib

    t, P = TORCH[dtype], _lib.ptr
    b, k = ni_d.shape
    ls_d = to_dev(np.atleast_1d(ls), t)
    mode = (0, noise, None) if isinstance(noise, float) else (1 if noise.ndim == 1 else 2, 0.0, P(noise))
    g_l = torch.full((b, ls_d.numel()), sentinel, device="cuda", dtype=t) if "ls" in want else None
    g_n = torch.full((b, k), sentinel, device="cuda", dtype=t) if "noise" in want else None
    g_nu = torch.full((b,), sentinel, device="cuda", dtype=t) if "nu" in want else None
    info = torch.zeros(1, dtype=torch.int32, device="cuda")
    cot = [None if g is None else to_dev(g, t) for g in (gm, gv, gyk)]
    rc = _lib.fn("hyper_backward_gen_wave", t)(P(X_d), X_d.shape[1], P(bi_d), P(ni_d), b, k, P(Y_d), Y_d.shape[1], *mode, float(nu),
                                               {"l2": 0, "F2": 1}[metric], P(ls_d), ls_d.numel(), *[P(g) for g in cot],
                                               P(g_l), P(g_n), P(g_nu), P(info), _lib.stream_ptr())
    torch.cuda.synchronize()
    if rc == OK:
        assert _lib.last_kernel().startswith(NAME), _lib.last_kernel()
    return rc, g_l, g_n, g_nu, int(info.item())


# (k, d, nu, metric, aniso, noise, batch_idx, form, want, dtype)
CASES = [
    (1, 3, 1.3, "l2", False, "scalar", False, "loocv", ALL, "float64"),
    (2, 1, 1.0, "l2", True, "table", True, "posterior3", ALL, "float32"),
    (2, 8, 3.7, "F2", False, "batch", True, "loocv", ("ls", "nu"), "float64"),
    (29, 8, 1.3, "l2", True, "scalar", True, "loocv", ALL, "float64"),
    (29, 40, 0.3, "F2", False, "table", False, "posterior", ALL, "float32"),
    (30, 16, 1.3, "l2", True, "batch", True, "posterior3", ALL, "float64"),
    (30, 40, 1.3, "l2", False, "scalar", True, "loocv", ALL, "float32"),
    (30, 64, 1.0, "l2", True, "table", False, "loocv", ALL, "float32"),
    (30, 3, 0.3, "F2", True, "scalar", True, "loocv", ("ls",), "float64"),
    (30, 8, 8.0, "l2", False, "batch", False, "posterior", ("noise", "nu"), "float32"),
    (30, 1, 8.0, "l2", False, "scalar", True, "posterior3", ALL, "float64"),
    (31, 8, 1.3, "l2", True, "scalar", True, "loocv", ("ls", "noise"), "float64"),
    (31, 3, 0.3, "l2", False, "table", False, "posterior", ("ls",), "float64"),
    (31, 16, 3.7, "l2", True, "batch", True, "loocv", ALL, "float32"),
    (31, 40, 0.3, "F2", True, "scalar", False, "posterior3", ALL, "float32"),
    (61, 8, 1.0, "l2", False, "table", True, "loocv", ("ls", "noise"), "float64"),
    (61, 40, 1.3, "l2", True, "scalar", True, "posterior", ALL, "float32"),
    (62, 8, 1.3, "l2", True, "batch", False, "loocv", ("noise",), "float64"),
    (62, 3, 3.7, "l2", False, "scalar", True, "posterior3", ("ls", "nu"), "float32"),
    (62, 64, 1.3, "l2", True, "table", False, "loocv", ("ls", "noise"), "float32"),
    (62, 3, 0.3, "F2", False, "scalar", True, "loocv", ("ls", "noise"), "float64"),
    # refused by design: the forms whose instantiation would spill
    (31, 8, 1.3, "l2", False, "scalar", True, "loocv", ALL, "float64"),
    (62, 64, 1.3, "l2", False, "scalar", True, "loocv", ALL, "float32"),
    (40, 9, 1.3, "l2", False, "scalar", True, "loocv", ("ls",), "float64"),
]
REFUSED = {21, 22, 23}


@pytest.mark.parametrize("n", range(len(CASES)), ids=["-".join(map(str, c)).replace("'", "") for c in CASES])
def test_entry_against_the_reference(n):
    k, d, nu, metric, aniso, noise_mode, with_bi, form, want, dtype = CASES[n]
    rng = np.random.default_rng(1000 + n)
    b, rows_n = 5, 300
    gm, gv, gyk, R = cotangents(rng, form, b)
    X, Y = make_table(rng, rows_n, d, R)
    ni = neighbourhoods(rng, rows_n, b, k)
    bi = rng.choice(rows_n, size=b, replace=False) if with_bi else np.arange(b)
    ls = scales(rng, d, aniso)
    table = NUGGET * (1.0 + rng.uniform(size=rows_n))
    rows = np.full((b, k), NUGGET) if noise_mode == "scalar" else table[ni]
    t = TORCH[dtype]
    noise = NUGGET if noise_mode == "scalar" else to_dev(table if noise_mode == "table" else rows, t)
    rc, *got, info = entry(dtype, to_dev(X, t), to_dev(bi) if with_bi else None, to_dev(ni), to_dev(Y, t), noise, nu, metric, ls,
                           gm, gv, gyk, want=want)
    assert rc == (EUNSUPPORTED if n in REFUSED else OK)
    if n in REFUSED:
        return
    assert info == 0 and [g is None for g in got] == [w not in want for w in ALL]
    check_partials(got, GR.partials(X, bi, ni, Y, rows, nu, metric, ls, gm, gv, gyk), dtype, nu, f"case {n}")


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("k", [12, 40])
def test_placement_bit_for_bit(k, dtype):
    """Alone, at an even and an odd position, and next to a partner whose points are the same ones scaled by 1e-3: its
    distances are tiny and its node count far larger -- what a wave-wide node count would let leak."""
    rng = np.random.default_rng(k)
    n, d = 200, 8
    X, Y = make_table(rng, n, d)
    X = np.concatenate([X, 1e-3 * X])
    Y = np.concatenate([Y, Y])
    ni = neighbourhoods(rng, n, 4, k)
    bi = rng.choice(n, size=4, replace=False)
    ni[1], bi[1] = ni[0] + n, bi[0] + n  # the scaled copy of neighbourhood 0
    gm, gv, gyk, _ = cotangents(rng, "loocv", 4)
    want = ("ls", "noise") if (dtype, k) == ("float64", 40) else ALL  # (fp64 beyond 32 slots: no grad_nu form)
    t = TORCH[dtype]
    Xd, Yd = to_dev(X, t), to_dev(Y, t)

    def run(order):
        o = np.asarray(order)
        rc, *got, info = entry(dtype, Xd, to_dev(bi[o]), to_dev(ni[o]), Yd, NUGGET, 1.3, "l2", length_scales(np.random.default_rng(0), d, True),
                               gm[o], gv[o], gyk[o], want=want)
        assert rc == OK and info == 0
        return [g.cpu().numpy() for g in got if g is not None]

    alone = run([0])
    assert all(np.isfinite(a).all() for a in alone)
    for order, pos in (([0, 2, 3], 0), ([2, 0, 3], 1), ([2, 3, 0], 2), ([0, 1], 0), ([1, 0], 1), ([2, 3, 1, 0], 3)):
        for a, g in zip(alone, run(order)):
            assert a[0].tobytes() == g[pos].tobytes(), (order, a[0], g[pos])


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_a_singular_neighbourhood_counts_once_and_spares_its_partner(dtype):
    rng = np.random.default_rng(6)
    n, d, k, b = 300, 8, 12, 4
    X, Y = make_table(rng, n, d)
    ni, bi = neighbourhoods(rng, n, b, k), rng.choice(n, size=b, replace=False)
    ni[1, 1] = ni[1, 0]   # a neighbour twice, at an odd position ...
    noise = np.full((b, k), NUGGET)
    noise[1] = 0.0        # ... and no nugget: exactly singular
    good = np.array([0, 2, 3])
    gm, gv, gyk, _ = cotangents(rng, "loocv", b)
    ls = length_scales(rng, d, False)
    ref = GR.partials(X, bi[good], ni[good], Y, noise[good], 1.3, "l2", ls, gm[good], gv[good], gyk[good])
    t = TORCH[dtype]
    rc, *got, info = entry(dtype, to_dev(X, t), to_dev(bi), to_dev(ni), to_dev(Y, t), to_dev(noise, t), 1.3, "l2", ls, gm, gv, gyk,
                           sentinel=-777.0)
    assert rc == OK and info == 1
    assert all((g[1] == -777.0).all() for g in got)
    check_partials([g[to_dev(good)] for g in got], ref, dtype, 1.3, "the partner and the others")


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("nu, aniso", [(0.3, False), (1.0, True)])
def test_pairs_at_zero_distance_contribute_nothing(nu, aniso, dtype):
    rng = np.random.default_rng(8)
    n, d, k, b = 300, 3, 20, 5
    X, Y = make_table(rng, n, d)
    ni, bi = neighbourhoods(rng, n, b, k), rng.choice(n, size=b, replace=False)
    ni[:, 1] = ni[:, 0]      # a neighbour twice
    ni[::2, 5] = bi[::2]     # the query among its own neighbours
    ls = length_scales(rng, d, aniso)
    gm, gv, gyk, _ = cotangents(rng, "loocv", b)
    ref = GR.partials(X, bi, ni, Y, np.full((b, k), NUGGET), nu, "l2", ls, gm, gv, gyk)
    t = TORCH[dtype]
    rc, *got, info = entry(dtype, to_dev(X, t), to_dev(bi), to_dev(ni), to_dev(Y, t), NUGGET, nu, "l2", ls, gm, gv, gyk)
    assert rc == OK and info == 0
    check_partials(got, ref, dtype, nu, f"duplicates, nu = {nu}")


def _loocv_args(k, d=4, t=torch.float64, b=48):
    X, y, bi, ni = _functor_problem(31 + k, 800, b, k, d, np.full(d, 1.2))
    return to_dev(X, t), to_dev(y, t), to_dev(bi), to_dev(ni)


def test_the_switch_serves_the_loocv_gradient_and_hands_refused_shapes_on():
    from muygpys_amd import _lib, fused

    args = _loocv_args(30)
    spec = lambda ls=1.4, noise=1e-2, nu=1.3: fused.KernelSpec("matern_gen", "l2", ls, noise, smoothness=nu)  # noqa: E731
    assert fused.gen_backward_default() == "slab"
    with pytest.raises(ValueError, match="gen_backward"):
        with fused.gen_backward("wave"):
            pass
    with fused.gen_backward("wavefront"):
        got = fused.loocv_value_and_grad(spec(), *args, grad_smoothness=True)
        assert _lib.last_kernel().startswith(NAME + "double,32,"), _lib.last_kernel()

        def f(**kw):
            return fused.loocv_value_and_grad(spec(**kw), *args)[0]

        fd = np.array([(f(ls=1.4 + 1e-5) - f(ls=1.4 - 1e-5)) / 2e-5, (f(noise=1e-2 + 1e-5) - f(noise=1e-2 - 1e-5)) / 2e-5,
                       (f(nu=1.3 + 1e-5) - f(nu=1.3 - 1e-5)) / 2e-5])
        # shapes the kernel refuses: the next rung serves the call
        for k, d, dt, name in ((63, 4, torch.float32, "mgp::backward_gen_kernel<float"), (30, 17, torch.float64, "mgp::backward_gen_kernel<double")):
            out = fused.loocv_value_and_grad(spec(), *_loocv_args(k, d, dt, b=8), grad_smoothness=True)
            assert _lib.last_kernel().startswith(name), _lib.last_kernel()
            assert all(np.isfinite(np.asarray(g, dtype=np.float64)).all() for g in out)
    flat = np.array([float(np.asarray(got[1]).reshape(-1)[0]), float(got[2]), float(got[3])])
    print(f"wavefront {flat!r}, central differences {fd!r}")
    np.testing.assert_allclose(flat, fd, rtol=2e-6, atol=2e-7 * np.abs(fd).max())


def test_lbfgsb_with_a_free_smoothness_ends_at_the_slab_modes_optimum():
    from muygpys_amd import fused
    from muygpys_amd.optimize import L_BFGS_B_optimize
    from tests.test_gpu_gen_backward import _gen_model

    X, y, bi, ni = _functor_problem(4, 2000, 150, 30, 3, np.full(3, 1.1))
    Xd, yd = to_dev(X, torch.float64), to_dev(y, torch.float64)
    ends = {}
    for mode in ("slab", "wavefront"):
        m = _gen_model(1.0, 2.0, noise=1e-3)
        cross, pair, y_b, y_nn = m.make_train_tensors(to_dev(bi), to_dev(ni), Xd, yd)
        with fused.gen_backward(mode):
            new = L_BFGS_B_optimize(m, y_b, y_nn, cross, pair, analytic_gradient=True)
        ends[mode] = (float(new.kernel.deformation.length_scale()), float(new.kernel.smoothness()))
    print(f"(length scale, nu): {ends!r}")
    np.testing.assert_allclose(ends["wavefront"], ends["slab"], rtol=1e-4)
