"""GPU: the whole posterior backward beyond LDS (csrc/mgp_backward_large_full.hip: ``mgp_posterior_backward_large_*`` on
the slab factor) -- feature, response, length-scale and noise cotangents against the fp64 oracle
(``orc.posterior_vjp``; the per-neighbourhood partials from ``reference_partials`` of tests/test_gpu_large_backward.py)
at every block and tile edge through the C entry, beyond the LDS backward through
``autograd.posterior(beyond_lds=True)``, against central differences of the forward, against the LDS backward where
both serve, placement, zero distances, failure semantics, the layers and the limits.

Inputs as tests/test_gpu_large_backward.py.  Tolerances: the project's for gradients -- fp64 1e-5, fp32 3 x 1e-3 -- through
tests/util.assert_close, over the rows a case references (the other rows of a gradient table must be exactly 0)."""

import numpy as np
import pytest
import torch

from oracle import muygps_oracle as orc
from tests.test_gpu_large_backward import (GRAD_RTOL, KERNELS, LS, NUGGET, TORCH, length_scales, limit, make_table,
                                           neighbourhoods, reference_partials)
from tests.util import assert_close, to_dev

pytestmark = pytest.mark.gpu

OUTPUTS = {"all": ("q", "x", "t", "ls", "noise"), "features": ("q", "x"), "targets": ("t",), "hyper": ("ls", "noise")}
KERNEL_NAME = {"float32": "mgp::posterior_backward_large_kernel<float>", "float64": "mgp::posterior_backward_large_kernel<double>"}


# ---- the C entry -------------------------------------------------------------------------------------------------------
def entry(dtype, Xq_d, Xn_d, bi_d, ni_d, Y_d, noise, kernel, metric, ls, gm, gv, want=OUTPUTS["all"], workspace=None,
          sentinel=0.0, lds=False):
    """One ``mgp_posterior_backward_large_*`` call (``lds``: ``mgp_posterior_backward_*``, the same arguments without a
    workspace).  ``Xq_d is Xn_d``: one shared gradient buffer for both roles.  ``noise``: a float, a (n,) table or a
    (b, k) tensor on the device.  Returns a dict of the outputs asked for (feature and response tables zero-filled,
    grad_ls / grad_noise pre-filled with ``sentinel``) and ``info``."""
    from muygpys_amd import _lib
    from muygpys_amd.fused import KernelSpec

    t = TORCH[dtype]
    lib, P = _lib.load(), _lib.ptr
    b, k = ni_d.shape
    d, R = Xn_d.shape[1], Y_d.shape[1]
    spec = KernelSpec(kernel, metric, 1.0, 0.0)
    ls_d = to_dev(np.atleast_1d(ls), t)
    mode = (0, noise, None) if isinstance(noise, float) else (1 if noise.ndim == 1 else 2, 0.0, P(noise))
    out = dict.fromkeys(("q", "x", "t", "ls", "noise"))
    if "x" in want:
        out["x"] = torch.zeros_like(Xn_d)
    if "q" in want:
        out["q"] = out["x"] if Xq_d is Xn_d and out["x"] is not None else torch.zeros_like(Xq_d)
    if "t" in want:
        out["t"] = torch.zeros_like(Y_d)
    if "ls" in want:
        out["ls"] = torch.full((b, ls_d.numel()), sentinel, device="cuda", dtype=t)
    if "noise" in want:
        out["noise"] = torch.full((b, k), sentinel, device="cuda", dtype=t)
    info = torch.zeros(1, dtype=torch.int32, device="cuda")
    cot = [None if g is None else to_dev(g, t) for g in (gm, gv)]
    args = (P(Xq_d), P(Xn_d), d, P(bi_d), P(ni_d), b, k, P(Y_d), R, *mode, spec.kernel_id(), spec.metric_id(), P(ls_d),
            ls_d.numel(), *[P(g) for g in cot], *[P(out[n]) for n in ("q", "x", "t", "ls", "noise")], P(info))
    if lds:
        rc = _lib.fn("posterior_backward", t)(*args, _lib.stream_ptr())
    else:
        if workspace is None:
            workspace = torch.empty(lib.mgp_backward_large_workspace_bytes(Xn_d.element_size(), k, b), dtype=torch.uint8, device="cuda")
        rc = _lib.fn("posterior_backward_large", t)(*args, P(workspace), workspace.numel(), _lib.stream_ptr())
    assert rc == 0, rc
    torch.cuda.synchronize()
    if not lds:
        assert _lib.last_kernel() == KERNEL_NAME[dtype]
    out["info"] = int(info.item())
    return out


# ---- the fp64 reference ------------------------------------------------------------------------------------------------
def reference(kernel, metric, ls, noise, rows, Xq, Xn, bi, ni, Y, gm, gv, shared=False):
    """fp64: the tables ``q`` / ``x`` / ``t`` of ``orc.posterior_vjp`` (``shared``: q and x added into one table) and the
    per-neighbourhood partials ``ls`` (b, ls_count) / ``noise`` (b, k) of ``reference_partials`` -- which knows one
    table, so the queries are appended to the training rows.  ``noise``: what the oracle's Spec takes (a scalar or the
    (n,) table); ``rows``: the (b, k) diagonal."""
    b, R = len(bi), Y.shape[1]
    gm0 = np.zeros((b, R)) if gm is None else gm
    gv0 = np.zeros(b) if gv is None else gv
    vjp = orc.posterior_vjp(orc.Spec(kernel, metric, ls, noise), Xq, Xn, bi, ni, Y, gm0, gv0)
    p_ls, p_n = reference_partials(orc.Spec(kernel, metric, ls, 0.0), np.concatenate([Xn, Xq]), len(Xn) + bi, ni, Y, rows, gm, gv, None)
    np.testing.assert_allclose(p_ls.sum(0), vjp["length_scale"], rtol=1e-8, atol=1e-10 * (1.0 + np.abs(p_ls).sum()))
    q, x = vjp["test_features"], vjp["train_features"]
    return dict(q=q + x if shared else q, x=q + x if shared else x, t=vjp["targets"], ls=p_ls, noise=p_n)


def check(got, ref, dtype, what, bi, ni, shared=False):
    """Every output asked for against the reference: tables over the rows the case references, the others exactly 0."""
    used = dict(q=np.unique(np.concatenate([bi, ni.ravel()]) if shared else bi),
                x=np.unique(np.concatenate([bi, ni.ravel()]) if shared else ni), t=np.unique(ni))
    for name in ("q", "x", "t", "ls", "noise"):
        if got[name] is None:
            continue
        g, r = got[name].double().cpu().numpy(), ref[name]
        if name in used:
            mask = np.zeros(len(g), dtype=bool)
            mask[used[name]] = True
            assert (g[~mask] == 0.0).all(), f"{what}: {name}: rows nobody references were written"
            g, r = g[mask], r[mask]
        assert np.isfinite(g).all(), f"{what}: {name}"
        print(f"{what}: {name} max |err| {np.abs(g - r).max():.3e}, rms(ref) {np.sqrt(np.mean(r * r)):.3e}")
        assert_close(g, r, GRAD_RTOL[dtype], f"{what}: {name}")


def cotangents(rng, form, b, R):
    return (None if form == "var" else rng.normal(size=(b, R))), (None if form == "mean" else rng.normal(size=b))


# ---- 1. block and tile edges at small size -----------------------------------------------------------------------------
# k and d as tests/test_gpu_large_backward.py (the panel edge, the fp64 tile edge, 126 / 127 on either side of the 256 /
# 512-thread switch; d = 70 takes two feature chunks); F2 goes with rbf and matern05 only.
EDGE_K = (1, 2, 31, 32, 33, 67, 96, 126, 127)
EDGE_D = (1, 3, 8, 40, 70)
EDGE_FORMS = ("mean", "var", "both")


def _edge_cases():
    rng = np.random.default_rng(20261020)
    n_cases = 30

    def spread(values):
        reps = -(-n_cases // len(values))
        return [values[i] for i in rng.permutation(np.tile(np.arange(len(values)), reps))[:n_cases]]

    cols = dict(k=spread(EDGE_K), d=spread(EDGE_D), kernel=spread(KERNELS), metric=spread(("l2", "F2")), aniso=spread((False, True)),
                noise=spread(("scalar", "table", "batch")), bi=spread((True, False)), shared=spread((False, True)),
                R=spread((1, 3)), form=spread(EDGE_FORMS), want=spread(tuple(OUTPUTS)), dtype=spread(("float32", "float64")))
    cases = [{name: vals[i] for name, vals in cols.items()} for i in range(n_cases)]
    # ... and the combinations at which the kernel takes a path of its own: either block size next to the switch in both
    # widths with per-feature scales, and two feature chunks in the sweep, one of them narrower than a group of pieces
    for j, (k, d, dtype) in enumerate([(126, 8, "float32"), (127, 8, "float32"), (126, 8, "float64"), (127, 8, "float64"),
                                       (33, 70, "float32"), (33, 70, "float64")]):
        base = dict(cases[j])
        base.update(k=k, d=d, dtype=dtype, aniso=True, kernel="matern15", want="all", form="both")
        cases.append(base)
    for c in cases:
        if c["kernel"] in ("matern15", "matern25", "maternInf"):
            c["metric"] = "l2"
    return cases


EDGE_CASES = _edge_cases()


def _edge_id(c):
    return (f"k{c['k']}-d{c['d']}-{c['kernel']}-{c['metric']}-{'aniso' if c['aniso'] else 'iso'}-{c['noise']}"
            f"-{'bi' if c['bi'] else 'nobi'}-{'shared' if c['shared'] else 'two'}-R{c['R']}-{c['form']}-{c['want']}-{c['dtype']}")


# (that the sample holds every value of every factor is asserted on the CPU: tests/test_large_full_backward_status_cpu.py)
@pytest.mark.parametrize("c", EDGE_CASES, ids=[_edge_id(c) for c in EDGE_CASES])
def test_block_and_tile_edges(c):
    rng = np.random.default_rng(sum(map(ord, _edge_id(c))))
    k, d, dtype, R, b, n = c["k"], c["d"], c["dtype"], c["R"], 5, 300
    gm, gv = cotangents(rng, c["form"], b, R)
    Xn, Y = make_table(rng, n, d, R)
    Xq = Xn if c["shared"] else rng.uniform(size=(n, d))
    ni = neighbourhoods(rng, n, b, k)
    bi = rng.choice(n, size=b, replace=False) if c["bi"] else np.arange(b)
    ls = length_scales(rng, d, c["aniso"])
    table = NUGGET * (1.0 + rng.uniform(size=n))
    t = TORCH[dtype]
    if c["noise"] == "scalar":
        rows, noise, onoise = np.full((b, k), NUGGET), NUGGET, NUGGET
    else:
        rows, noise, onoise = table[ni], to_dev(table if c["noise"] == "table" else table[ni], t), table
    ref = reference(c["kernel"], c["metric"], ls, onoise, rows, Xq, Xn, bi, ni, Y, gm, gv, shared=c["shared"])
    Xn_d = to_dev(Xn, t)
    Xq_d = Xn_d if c["shared"] else to_dev(Xq, t)
    got = entry(dtype, Xq_d, Xn_d, to_dev(bi) if c["bi"] else None, to_dev(ni), to_dev(Y, t), noise, c["kernel"], c["metric"], ls,
                gm, gv, want=OUTPUTS[c["want"]])
    assert got["info"] == 0
    assert {n_ for n_ in OUTPUTS["all"] if got[n_] is not None} == set(OUTPUTS[c["want"]])
    check(got, ref, dtype, _edge_id(c), bi, ni, shared=c["shared"])


# ---- 2. beyond the LDS backward, through autograd ----------------------------------------------------------------------
def entries_called(monkeypatch):
    """The C entries asked for from here on, by base name (autograd runs ``backward`` on a thread of its own, and
    ``_lib.last_kernel()`` is per thread: the backward launch is told by the entry it went through)."""
    from muygpys_amd import _lib

    called, fn = [], _lib.fn
    monkeypatch.setattr(_lib, "fn", lambda base, dtype: (called.append(base), fn(base, dtype))[1])
    return called


RANGE_CASES = [("float32", "limit+1", 8, 1, True, False), ("float64", "limit+1", 8, 1, False, True), ("float32", 300, 6, 1, False, False),
               ("float64", 520, 4, 1, True, False), ("float32", 1020, 2, 3, False, False)]


@pytest.mark.parametrize("dtype, k, b, R, aniso, shared", RANGE_CASES,
                         ids=[f"{c[0]}-k{c[1]}-R{c[3]}-{'aniso' if c[4] else 'iso'}-{'shared' if c[5] else 'two'}" for c in RANGE_CASES])
def test_autograd_beyond_the_lds_backward(dtype, k, b, R, aniso, shared, monkeypatch):
    from muygpys_amd import _lib, autograd, fused

    k = limit(dtype) + 1 if k == "limit+1" else k
    rng = np.random.default_rng(k + 11)
    n, d = 1500, 8
    Xn, Y = make_table(rng, n, d, R)
    Xq = Xn if shared else rng.uniform(size=(n, d))
    ni, bi = neighbourhoods(rng, n, b, k), rng.choice(n, size=b, replace=False)
    ls = length_scales(rng, d, aniso)
    gm, gv = rng.normal(size=(b, R)), rng.normal(size=b)
    t = TORCH[dtype]
    x = to_dev(Xn, t).requires_grad_(True)
    q = x if shared else to_dev(Xq, t).requires_grad_(True)
    y = to_dev(Y, t).requires_grad_(True)
    ls_t = to_dev(np.atleast_1d(ls), t).requires_grad_(True)
    nz_t = torch.tensor(NUGGET, device="cuda", dtype=t, requires_grad=True)
    called = entries_called(monkeypatch)
    mean, var = autograd.posterior(fused.KernelSpec("matern15", "l2", ls_t, nz_t), q, x, to_dev(bi), to_dev(ni), y, beyond_lds=True)
    if k > _lib.load().mgp_max_nn_count(x.element_size(), R):
        assert _lib.last_kernel().startswith("mgp::fused_large_kernel<")
    ((mean * to_dev(gm, t)).sum() + (var * to_dev(gv, t)).sum()).backward()
    assert "posterior_backward_large" in called and "posterior_backward" not in called, called
    vjp = orc.posterior_vjp(orc.Spec("matern15", "l2", ls, NUGGET), Xq, Xn, bi, ni, Y, gm, gv)
    both = np.unique(np.concatenate([bi, ni.ravel()]))
    pairs = [("targets", y.grad, vjp["targets"], np.unique(ni))]
    if shared:
        pairs.append(("x.grad = train + test", x.grad, vjp["train_features"] + vjp["test_features"], both))
    else:
        pairs += [("train_features", x.grad, vjp["train_features"], np.unique(ni)), ("test_features", q.grad, vjp["test_features"], np.unique(bi))]
    for name, g, r, used in pairs:
        g = g.double().cpu().numpy()
        mask = np.zeros(len(g), dtype=bool)
        mask[used] = True
        assert (g[~mask] == 0.0).all(), name
        print(f"{name}: max |err| {np.abs(g[mask] - r[mask]).max():.3e}, rms(ref) {np.sqrt(np.mean(r[mask] ** 2)):.3e}")
        assert_close(g[mask], r[mask], GRAD_RTOL[dtype], name)
    print(f"length scale {ls_t.grad.cpu().numpy()!r} against {vjp['length_scale']!r}; noise {float(nz_t.grad)!r} against {vjp['noise']!r}")
    assert_close(ls_t.grad.double().cpu().numpy(), vjp["length_scale"], GRAD_RTOL[dtype], "length_scale")
    assert_close([float(nz_t.grad)], [vjp["noise"]], GRAD_RTOL[dtype], "noise")


# ---- 3. against central differences of the forward ---------------------------------------------------------------------
def test_feature_gradient_is_the_central_difference_of_the_forward():
    """fp64 at the first nn_count the LDS backward refuses, d = 4: six feature coordinates -- of a neighbour row, of a
    query row and of a row two neighbourhoods share -- with rtol = 2e-6, atol = 2e-7 max |fd|, as
    tests/test_gpu_large_backward.py."""
    from muygpys_amd import autograd, fused

    k, d, b, n = limit("float64") + 1, 4, 4, 600
    rng = np.random.default_rng(97)
    Xn, Y = make_table(rng, n, d)
    Xq = rng.uniform(size=(b, d))
    ni = neighbourhoods(rng, n, b, k)
    twice = ni[0, 3]
    if twice not in ni[1]:
        ni[1, 5] = twice
    alone = next(r for r in ni[2] if (ni == r).sum() == 1)
    gm, gv = rng.normal(size=(b, 1)), rng.normal(size=b)
    t = torch.float64
    spec = fused.KernelSpec("matern15", "l2", LS, NUGGET)
    ni_d, gm_d, gv_d, Y_d = to_dev(ni), to_dev(gm, t), to_dev(gv, t), to_dev(Y, t)

    def value(xq, xn):
        mean, var = fused.posterior_mean_var(spec, to_dev(xq, t), to_dev(xn, t), None, ni_d, Y_d, path="large", packed=False)
        return float(((mean.reshape(b, 1) * gm_d).sum() + (var * gv_d).sum()).item())

    x, q = to_dev(Xn, t).requires_grad_(True), to_dev(Xq, t).requires_grad_(True)
    mean, var = autograd.posterior(spec, q, x, None, ni_d, Y_d, beyond_lds=True)
    ((mean * gm_d).sum() + (var * gv_d).sum()).backward()
    coords = [("x", alone, 0), ("x", alone, 3), ("q", 1, 1), ("q", 3, 2), ("x", twice, 0), ("x", twice, 2)]
    h = 1e-5
    fd, an = [], []
    for which, r, c in coords:
        up, dn = [Xq.copy(), Xn.copy()], [Xq.copy(), Xn.copy()]
        up[which == "x"][r, c] += h
        dn[which == "x"][r, c] -= h
        fd.append((value(*up) - value(*dn)) / (2 * h))
        an.append(float((x if which == "x" else q).grad[r, c]))
    fd, an = np.array(fd), np.array(an)
    print(f"analytic {an!r} against central differences {fd!r}")
    assert np.abs(fd).min() > 0
    np.testing.assert_allclose(an, fd, rtol=2e-6, atol=2e-7 * np.abs(fd).max())


# ---- 4. agreement where both serve -------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype, k", [("float32", 20), ("float64", 20), ("float32", 70), ("float64", 70), ("float32", 120)])
def test_agrees_with_the_lds_backward(dtype, k):
    rng = np.random.default_rng(k + 1)
    n, d, b, R = 1500, 8, 8, 2
    Xn, Y = make_table(rng, n, d, R)
    Xq = rng.uniform(size=(n, d))
    ni, bi = neighbourhoods(rng, n, b, k), rng.choice(n, size=b, replace=False)
    ls = length_scales(rng, d, True)
    gm, gv = rng.normal(size=(b, R)), rng.normal(size=b)
    t = TORCH[dtype]
    args = (dtype, to_dev(Xq, t), to_dev(Xn, t), to_dev(bi), to_dev(ni), to_dev(Y, t), NUGGET, "matern15", "l2", ls, gm, gv)
    got, ref = entry(*args), entry(*args, lds=True)
    assert got["info"] == 0 and ref["info"] == 0
    check(got, {n_: ref[n_].double().cpu().numpy() for n_ in OUTPUTS["all"]}, dtype, f"large vs LDS backward, k = {k}", bi, ni)


# ---- 5. placement ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_placement_invariance_bitwise(dtype):
    from muygpys_amd import _lib

    rng = np.random.default_rng(301)
    n, d, k, b = 1200, 8, 300, 9
    Xn, Y = make_table(rng, n, d)
    Xq = rng.uniform(size=(n, d))
    ni, bi = neighbourhoods(rng, n, b, k), rng.choice(n, size=b, replace=False)
    ls = length_scales(rng, d, True)
    gm, gv = rng.normal(size=(b, 1)), rng.normal(size=b)
    t = TORCH[dtype]
    Xq_d, Xn_d, Y_d = to_dev(Xq, t), to_dev(Xn, t), to_dev(Y, t)
    slab = _lib.load().mgp_backward_large_workspace_bytes(Xn_d.element_size(), k, 1)

    def run(rows, slabs=None, fill=0xFF):
        rows = np.asarray(rows)
        size = _lib.load().mgp_backward_large_workspace_bytes(Xn_d.element_size(), k, len(rows)) if slabs is None else slabs * slab
        ws = torch.empty(size, dtype=torch.uint8, device="cuda")
        ws.fill_(fill)  # (0xFF: NaN in every element, either width)
        got = entry(dtype, Xq_d, Xn_d, to_dev(bi[rows]), to_dev(ni[rows]), Y_d, NUGGET, "matern15", "l2", ls, gm[rows], gv[rows], workspace=ws)
        assert got["info"] == 0
        return {n_: got[n_].cpu().numpy() for n_ in OUTPUTS["all"]}

    alone = run([0], fill=0x00)
    assert all(np.isfinite(v).all() for v in alone.values())
    for name, got, pos in (("first of 9", run([0, 1, 2, 3, 4, 5, 6, 7, 8]), 0), ("last of 9", run([1, 2, 3, 4, 5, 6, 7, 8, 0]), 8),
                           ("one slab", run([3, 4, 0, 5, 6], 1), 2), ("0xFF", run([0]), 0)):
        for what in ("ls", "noise"):
            assert alone[what][0].tobytes() == got[what][pos].tobytes(), (name, what, alone[what][0], got[what][pos])
    # a batch of one neighbourhood: one atomic per address, so the accumulated tables are the same bits too
    again = run([0])
    for what in ("q", "x", "t"):
        assert alone[what].tobytes() == again[what].tobytes(), what


# ---- 6. zero distance --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("case", ["query among its neighbours", "two neighbours are one row", "d = 1"])
def test_zero_distances_take_the_zero_subgradient(case, dtype):
    """The two cases in three dimensions run at the first nn_count beyond the LDS backward.  The one-dimensional case
    runs at k = 33 (two panels: what handles a zero distance does not depend on k), where the comparison in the fp32
    band was checked on the CPU: 138 of 400 uniform points on the unit interval at length scale 0.5 give cond(K) = 1e4,
    and cond x eps(fp32) = 6e-4 leaves the 3e-3 band a factor of five.  Measured there in fp32 (k = 138, the worst
    element of grad_noise in units of the band): torch on the CPU 0.28, an unblocked fp32 Cholesky in numpy 0.32 - 0.46,
    the LDS backward at k = 137 0.54 - 0.70, the slab factor at k = 137 / 138 0.72 - 1.23 (up to 2 of 552 elements outside; the same
    bits from mgp_hyper_backward_large_*, so from phases 1 - 3); the feature gradients stay below 0.42."""
    rng = np.random.default_rng(len(case))
    n, b = 400, 4
    k = 33 if case == "d = 1" else limit(dtype) + 1
    d = 1 if case == "d = 1" else 3
    X, Y = make_table(rng, n, d)
    ni, bi = neighbourhoods(rng, n, b, k), rng.choice(n, size=b, replace=False)
    if case == "query among its neighbours":
        ni[:, 2] = bi
    else:
        X[ni[:, 1]] = X[ni[:, 0]]  # (distinct rows of the table at distance zero; the nugget keeps the system SPD)
    gm, gv = rng.normal(size=(b, 1)), rng.normal(size=b)
    t = TORCH[dtype]
    ref = reference("matern15", "l2", LS, NUGGET, np.full((b, k), NUGGET), X, X, bi, ni, Y, gm, gv, shared=True)
    X_d = to_dev(X, t)
    got = entry(dtype, X_d, X_d, to_dev(bi), to_dev(ni), to_dev(Y, t), NUGGET, "matern15", "l2", LS, gm, gv)
    assert got["info"] == 0
    check(got, ref, dtype, case, bi, ni, shared=True)


# ---- 7. failure semantics ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_singular_neighbourhoods_are_counted_and_issue_nothing(dtype):
    rng = np.random.default_rng(6)
    n, d, k, b = 1000, 8, 200, 8
    Xn, Y = make_table(rng, n, d)
    Xq = rng.uniform(size=(n, d))
    ni, bi = neighbourhoods(rng, n, b, k), rng.choice(n, size=b, replace=False)
    broken = np.array([2, 7])
    ni[broken, 1] = ni[broken, 0]  # a duplicated neighbour ...
    noise = np.full((b, k), NUGGET)
    noise[broken] = 0.0            # ... and no nugget: exactly singular
    good = np.setdiff1d(np.arange(b), broken)
    gm, gv = rng.normal(size=(b, 1)), rng.normal(size=b)
    ref = reference("matern15", "l2", LS, NUGGET, noise[good], Xq, Xn, bi[good], ni[good], Y, gm[good], gv[good])
    t, sentinel = TORCH[dtype], -777.0
    got = entry(dtype, to_dev(Xq, t), to_dev(Xn, t), to_dev(bi), to_dev(ni), to_dev(Y, t), to_dev(noise, t), "matern15", "l2", LS,
                gm, gv, sentinel=sentinel)
    assert got["info"] == 2
    assert (got["ls"][to_dev(broken)] == sentinel).all() and (got["noise"][to_dev(broken)] == sentinel).all()
    got["ls"], got["noise"] = got["ls"][to_dev(good)], got["noise"][to_dev(good)]
    check(got, ref, dtype, "the six good neighbourhoods", bi[good], ni[good])


# ---- 8. the layers -----------------------------------------------------------------------------------------------------
def _layer_problem(b, k, R, seed):
    rng = np.random.default_rng(seed)
    n, d_in = 600, 6
    X, Y = make_table(rng, n, d_in, R)
    bi = rng.choice(n, size=b, replace=False)
    ni = np.stack([rng.choice(np.delete(np.arange(n), i), size=k, replace=False) for i in bi])
    return X, Y, bi, ni


def _model(ls):
    from muygpys_amd.gp import MuyGPS
    from muygpys_amd.gp.deformation import Isotropy, l2
    from muygpys_amd.gp.hyperparameter import ScalarParam
    from muygpys_amd.gp.kernels import Matern
    from muygpys_amd.gp.noise import HomoscedasticNoise

    return MuyGPS(kernel=Matern(smoothness=ScalarParam(1.5), deformation=Isotropy(l2, length_scale=ScalarParam(ls))),
                  noise=HomoscedasticNoise(NUGGET))


def test_layer_trains_an_embedding_beyond_the_lds_backward(monkeypatch):
    from muygpys_amd.torch import MuyGPs_layer

    b, k, d_out = 32, limit("float32") + 1, 4
    X, Y, bi, ni = _layer_problem(b, k, 1, 8)
    t = torch.float32
    X_d, Y_d, bi_d, ni_d = to_dev(X, t), to_dev(Y, t), to_dev(bi), to_dev(ni)
    torch.manual_seed(0)
    embedding = torch.nn.Linear(X.shape[1], d_out).cuda()
    with pytest.raises(ValueError, match="exceeds the differentiable kernel's limit"):
        MuyGPs_layer(_model(LS), bi_d, ni_d, Y_d[bi_d], Y_d[ni_d])(embedding(X_d))
    layer = MuyGPs_layer(_model(LS), bi_d, ni_d, Y_d[bi_d], Y_d[ni_d], beyond_lds=True)
    opt = torch.optim.Adam(embedding.parameters(), lr=1e-2)
    before = embedding.weight.detach().clone()
    rng = np.random.default_rng(9)
    gm, gv = rng.normal(size=(b, 1)), rng.normal(size=b)
    called = entries_called(monkeypatch)
    pred, var = layer(embedding(X_d))
    assert pred.shape == (b, 1) and var.shape == (b,)
    ((pred * to_dev(gm, t)).sum() + (var * to_dev(gv, t)).sum()).backward()
    assert "posterior_backward_large" in called and "posterior_backward" not in called, called
    # the chain rule on the oracle's feature gradient: z = x W^T + c  ->  dW = (dz)^T x
    W, c = embedding.weight.detach().double().cpu().numpy(), embedding.bias.detach().double().cpu().numpy()
    Z = X @ W.T + c
    vjp = orc.posterior_vjp(orc.Spec("matern15", "l2", LS, NUGGET), Z, Z, bi, ni, Y, gm, gv)
    gz = vjp["train_features"] + vjp["test_features"]
    assert_close(embedding.weight.grad.double().cpu().numpy(), gz.T @ X, GRAD_RTOL["float32"], "embedding weight gradient")
    # (the bias gradient is the column sum of gz, zero in exact arithmetic -- a translation changes no distance: each
    # of its terms inside the band is all that can be asked of the sum)
    used = np.unique(np.concatenate([bi, ni.ravel()]))
    slack = GRAD_RTOL["float32"] * (np.abs(gz[used]).sum(0) + len(used) * np.sqrt(np.mean(gz[used] ** 2)))
    assert (np.abs(embedding.bias.grad.double().cpu().numpy() - gz.sum(0)) <= slack).all()
    opt.step()
    assert not torch.equal(before, embedding.weight.detach())


def test_multivariate_layer_beyond_the_lds_backward():
    from muygpys_amd.torch import MultivariateMuyGPs_layer

    b, k = 8, limit("float32") + 1
    X, Y, bi, ni = _layer_problem(b, k, 2, 10)
    t = torch.float32
    Y_d, bi_d, ni_d = to_dev(Y, t), to_dev(bi), to_dev(ni)
    layer = MultivariateMuyGPs_layer([_model(LS), _model(2.0 * LS)], bi_d, ni_d, Y_d[bi_d], Y_d[ni_d], beyond_lds=True)
    x = to_dev(X, t).requires_grad_(True)
    pred, var = layer(x)
    assert pred.shape == (b, 2) and var.shape == (b, 2)
    (pred.sum() + var.sum()).backward()
    assert torch.isfinite(x.grad).all() and float(x.grad.abs().sum()) > 0


# ---- 9. the limits -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k, R", [(1023, 1), (1021, 3)])
def test_beyond_the_limit_is_an_error_that_names_it(k, R):
    from muygpys_amd import autograd, fused

    rng = np.random.default_rng(k)
    n, d, b = 1100, 4, 2
    X, Y = make_table(rng, n, d, R)
    x = to_dev(X, torch.float32).requires_grad_(True)
    with pytest.raises(ValueError, match="mgp_large_max_nn_count"):
        autograd.posterior(fused.KernelSpec("matern15", "l2", LS, NUGGET), x, x, to_dev(np.arange(b)), to_dev(neighbourhoods(rng, n, b, k)),
                           to_dev(Y, torch.float32), beyond_lds=True)
